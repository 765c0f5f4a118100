// ka_ens_fam.cpp -- host side of the ensemble consensus stage for a batch of families with the same number of members: the
// ka_ens_fam handle of the C ABI (ka_ens.cpp is the one-family form; the kernels are ka_ens_fam.hip).
//
// Every family gets what ka_ens_create + ka_ens_add_member + ka_ens_score_rows + ka_ens_consensus + ka_ens_confidence give
// it alone; the number of launches and synchronisations of a call depends on n_runs and on the number of candidate chunks,
// never on the number of families.  A member is uploaded once, as the packed rows ka_batch_rows hands out; its maps serve
// the walks and its own score (ka_ens_fam_score_members).
//
// The consensus counts the candidates of every family and every support level in ONE pass and one synchronisation, then
// writes them level by level, highest first: a level is cut into chunks of whole families of at most KA_ENS_CHUNK
// candidates (a larger family is a chunk of its own).  While the device writes chunk c + 1 into the other buffer, the families
// of chunk c are dealt from pinned memory to the host threads; a thread replays whole families (the level's candidates into
// the family's own union, ka_ens_union.h), and after the last chunk the column order and the fill of whole families.  A
// family's result depends on its own candidates alone, so not on the dealing.
//
// Every check runs on the host before anything is launched (ens_fam_check; ka_ens_fam_check is its public form) with the
// functions the one-family calls use (KaSeqSet::set, ka_msa_check_rows): a family is refused with the cause it is refused
// with alone.  The host-only parts (the check, ka_debug_ens_fam_consensus_host) need no context and no GPU.
#include "ka_ctx.h"
#include "ka_ens.h"
#include "ka_ens_union.h"
#include "ka_msa.h"

int ka_ctx_device_stream(ka_ctx* c, int* device, hipStream_t* stream);    // (library-internal: ka_api.cpp)

namespace {

const char* const kWhyRes = "residue indices must stay below 4096 (the reference's POAR key ri << 20 | rj aliases beyond)";

double ms_since(std::chrono::steady_clock::time_point t0)
{
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// the families and their sequences: fam_first ascends from 0, no family is empty, every family's lengths as ka_ens_create takes them
int ens_fam_check_seqs(const std::string& me, int n_fam, const int* fam_first, const int* lens)
{
        if (n_fam < 1 || !fam_first || !lens) return fail(me + ": bad arguments");
        if (fam_first[0] != 0) return fail(me + ": fam_first does not ascend from 0 to numseq");
        for (int f = 0; f < n_fam; f++) {
                if (fam_first[f + 1] < fam_first[f]) return fail(me + ": fam_first does not ascend from 0 to numseq");
                if (fam_first[f + 1] == fam_first[f]) return fail(me + ": empty family");
        }
        long long residues = 0;
        for (int f = 0; f < n_fam; f++) {
                const std::string fam = me + ": family " + std::to_string(f);
                KaSeqSet q;                                      // (host side only: nothing to release)
                if (q.set(fam.c_str(), fam_first[f + 1] - fam_first[f], lens + fam_first[f], KA_ENS_MAX_RES, kWhyRes)) return KA_FAIL;
                residues += q.T;
                if (residues > INT32_MAX) return fail(me + ": more than 2^31 - 1 residues in the batch");
        }
        return KA_OK;
}

// a packed batch on the host alone: the families, their sequences and their rows.  skip: a family with alnlens[f] < 0 has no
// rows in the batch (ka_ens_fam_score)
int ens_fam_check(const char* who, int n_fam, const int* fam_first, const int* lens, const uint8_t* rows, const int* alnlens, bool skip)
{
        const std::string me(who);
        if (!rows || !alnlens) return fail(me + ": bad arguments");
        if (ens_fam_check_seqs(me, n_fam, fam_first, lens)) return KA_FAIL;
        long long off = 0;
        for (int f = 0; f < n_fam; f++) {
                if (skip && alnlens[f] < 0) continue;
                const std::string fam = me + ": family " + std::to_string(f);
                const int N = fam_first[f + 1] - fam_first[f];
                KaSeqSet q;
                if (q.set(fam.c_str(), N, lens + fam_first[f], KA_ENS_MAX_RES, kWhyRes)) return KA_FAIL;
                if (ka_msa_check_rows(fam.c_str(), q, rows + off, (long long)alnlens[f] + 1, alnlens[f])) return KA_FAIL;
                off += (long long)N * (alnlens[f] + 1);
                if (off > INT32_MAX) return fail(me + ": more than 2^31 - 1 row bytes in the batch");
        }
        return KA_OK;
}

// a family's consensus: rows = N_f x W bytes.  build_families: families f0 .. f1 from whole candidate lists (family f: cand +
// 2 * candFirst[f]) on n_threads threads
struct FamResult {
        std::vector<uint8_t> rows;
        int W = 0;
        long long truncations = 0;
        double ms = 0.0;
};

bool build_families(int f0, int f1, int n_threads, const int* fam_first, const int* lens, const int* offs, const long long* candFirst, const int* cand,
                    const uint8_t* letters, std::vector<FamResult>& out)
{
        return ka_ens_deal(f0, f1, n_threads, [&](int f) {
                const auto t0 = std::chrono::steady_clock::now();
                FamResult& r = out[f];
                const int s0 = fam_first[f];
                KaEnsFamilyUnion u;
                u.init(fam_first[f + 1] - s0, lens + s0);
                u.join(cand + 2 * candFirst[f], candFirst[f + 1] - candFirst[f]);
                u.finish(letters + offs[s0], r.rows, &r.W);
                r.truncations = u.uf.truncations;
                r.ms = ms_since(t0);
        });
}

// the results packed as ka_batch_rows packs rows: the rows of family f W[f] + 1 bytes apart, a 0 byte after each
long long packed_size(const std::vector<FamResult>& res, const int* fam_first)
{
        long long n = 0;
        for (size_t f = 0; f < res.size(); f++) n += (long long)(fam_first[f + 1] - fam_first[f]) * (res[f].W + 1);
        return n;
}

void pack_rows(const std::vector<FamResult>& res, const int* fam_first, uint8_t* out)
{
        for (size_t f = 0; f < res.size(); f++) {
                const int N = fam_first[f + 1] - fam_first[f], W = res[f].W;
                for (int s = 0; s < N; s++) {
                        std::memcpy(out, res[f].rows.data() + (size_t)s * W, W);
                        out[W] = 0;
                        out += W + 1;
                }
        }
}

} // namespace

struct ka_ens_fam {
        int device = 0;
        hipStream_t stream = nullptr;
        int F = 0, S = 0, T = 0, R = 0, nBlocks = 0;
        long long E = 0;                                         // entries of one level of the count table
        long long chunkCap = 0;
        std::vector<int> famFirst, lens, offs, blkFirst;
        std::vector<KaEnsFam> fams;
        std::vector<uint8_t> added;                              // member k was added
        std::vector<int> memW, memCell;                          // [R][F], [R][F + 1]
        std::vector<long long> memRowOff;                        // [R][F]
        long long resBase[KA_ENS_MAX_RUNS] = {};
        bool mapsFresh = false;
        size_t ldsX = 0, ldsCand = 0;                            // the walk's LDS with and without an alignment X
        std::vector<DevBuf<uint8_t>> dRows;                      // member k's packed rows
        DevBuf<KaEnsFam> dFams;
        DevBuf<int> dFirstSeq, dBlkFirst, dOffs, dLens, dCol, dMemW, dMemCell, dColX, dXTab, dSup, dNp, dCnt;
        DevBuf<long long> dMemRowOff, dXRowOff, dPairOff, dRowTot, dRowBase;
        DevBuf<int16_t> dRes, dResX;
        DevBuf<uint8_t> dRowsX;
        DevBuf<unsigned long long> dScore;
        DevBuf<float> dConf, dColConf;
        DevBuf<int2> dOut[2];
        int2* pinned[2] = { nullptr, nullptr };
        long long pinnedCap = 0;
        hipEvent_t ready[2] = { nullptr, nullptr }, wBeg[2] = { nullptr, nullptr }, wEnd[2] = { nullptr, nullptr }, ev0 = nullptr, ev1 = nullptr;
        std::vector<FamResult> cons;                             // the last consensus
        bool haveCons = false;
        double st[KA_ENS_FAM_STATS] = {};
        int nLaunch = 0, nSync = 0;                              // of the call that is running

        ~ka_ens_fam()
        {
                for (int b = 0; b < 2; b++) {
                        if (pinned[b]) (void)hipHostFree(pinned[b]);
                        if (ready[b]) (void)hipEventDestroy(ready[b]);
                        if (wBeg[b]) (void)hipEventDestroy(wBeg[b]);
                        if (wEnd[b]) (void)hipEventDestroy(wEnd[b]);
                        dOut[b].release();
                }
                if (ev0) (void)hipEventDestroy(ev0);
                if (ev1) (void)hipEventDestroy(ev1);
                for (auto& r : dRows) r.release();
                dFams.release(); dFirstSeq.release(); dBlkFirst.release(); dOffs.release(); dLens.release(); dCol.release(); dMemW.release();
                dMemCell.release(); dColX.release(); dXTab.release(); dSup.release(); dNp.release(); dCnt.release();
                dMemRowOff.release(); dXRowOff.release(); dPairOff.release(); dRowTot.release(); dRowBase.release(); dRes.release(); dResX.release();
                dRowsX.release(); dScore.release(); dConf.release(); dColConf.release();
        }

        float evMs() { float m = 0.0f; (void)hipEventElapsedTime(&m, ev0, ev1); return m; }
        void begin() { nLaunch = nSync = 0; }
        void end(int slot) { st[slot] = nLaunch; st[slot + 1] = nSync; }

        KaEnsFamArgs args() const
        {
                KaEnsFamArgs a{};
                a.nFam = F; a.S = S; a.T = T; a.R = R; a.E = E;
                a.fams = dFams.p; a.firstSeq = dFirstSeq.p; a.blkFirst = dBlkFirst.p; a.offs = dOffs.p; a.lens = dLens.p;
                a.col = dCol.p; a.res = dRes.p; a.memCell = dMemCell.p; a.memW = dMemW.p;
                std::copy_n(resBase, KA_ENS_MAX_RUNS, a.resBase);
                return a;
        }

        int ensure_maps(const char* who);
        int maps_x(const char* who, const uint8_t* rows, const int* alnlens, KaEnsFamArgs& a, int* cells, int* cols);
        int scores_back(long long* sums_out, double* scores_out, int n);
        int consensus(const int* minSup, const uint8_t* letters, int nThreads);
};

// the members' maps: one maps launch per member over all families
int ka_ens_fam::ensure_maps(const char* who)
{
        if (mapsFresh) return KA_OK;
        for (int k = 0; k < R; k++)
                if (!added[k]) return fail(std::string(who) + ": member " + std::to_string(k) + " not added (all n_runs members are needed)");
        long long o = 0;
        for (int k = 0; k < R; k++) {
                resBase[k] = o;
                int c = 0;
                for (int f = 0; f < F; f++) { memCell[(size_t)k * (F + 1) + f] = c; c += fams[f].N * memW[(size_t)k * F + f]; }
                memCell[(size_t)k * (F + 1) + F] = c;
                o += c;
        }
        if (dCol.alloc((size_t)R * std::max(T, 1)) || dRes.alloc((size_t)o)) return fail(std::string(who) + ": out of device memory (maps)");
        HIPCHK(hipMemcpyAsync(dMemW.p, memW.data(), sizeof(int) * memW.size(), hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(dMemCell.p, memCell.data(), sizeof(int) * memCell.size(), hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(dMemRowOff.p, memRowOff.data(), sizeof(long long) * memRowOff.size(), hipMemcpyHostToDevice, stream));
        HIPCHK(hipEventRecord(ev0, stream));
        const KaEnsFamArgs a = args();
        for (int k = 0; k < R; k++) {
                ka_ensf_launch_maps(a, dRows[k].p, dMemRowOff.p + (size_t)k * F, dMemW.p + (size_t)k * F, dMemCell.p + (size_t)k * (F + 1),
                                    dCol.p + (long long)k * T, dRes.p + resBase[k], stream);
                nLaunch++;
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev1, stream));
        HIPCHK(hipEventSynchronize(ev1));
        nSync++;
        st[0] = evMs();
        mapsFresh = true;
        return KA_OK;
}

// the alignments X of a score / confidence call (alnlens[f] < 0: none for family f): one upload, their maps in dColX / dResX
int ka_ens_fam::maps_x(const char* who, const uint8_t* rows, const int* alnlens, KaEnsFamArgs& a, int* cells, int* cols)
{
        // xW [F] | xCell [F + 1] | xCol [F + 1]
        std::vector<int> tab((size_t)3 * F + 2);
        std::vector<long long> rowOff(F);
        int* xW = tab.data();
        int* xCell = xW + F;
        int* xCol = xCell + F + 1;
        long long ro = 0;
        int c = 0, w = 0;
        for (int f = 0; f < F; f++) {
                const int W = std::max(alnlens[f], 0);
                xW[f] = W; xCell[f] = c; xCol[f] = w; rowOff[f] = ro;
                c += fams[f].N * W;
                w += W;
                if (W > 0) ro += (long long)fams[f].N * (W + 1);
        }
        xCell[F] = c; xCol[F] = w;
        if (dRowsX.alloc((size_t)std::max(ro, 1LL)) || dColX.alloc((size_t)std::max(T, 1)) || dResX.alloc((size_t)std::max(c, 1)))
                return fail(std::string(who) + ": out of device memory");
        if (ro) HIPCHK(hipMemcpyAsync(dRowsX.p, rows, (size_t)ro, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(dXTab.p, tab.data(), sizeof(int) * tab.size(), hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(dXRowOff.p, rowOff.data(), sizeof(long long) * F, hipMemcpyHostToDevice, stream));
        HIPCHK(hipStreamSynchronize(stream));                    // (rows, tab and rowOff are read until here)
        nSync++;
        a.colX = dColX.p; a.resX = dResX.p; a.xW = dXTab.p; a.xCell = dXTab.p + F; a.xCol = dXTab.p + 2 * F + 1;
        ka_ensf_launch_maps(a, dRowsX.p, dXRowOff.p, a.xW, a.xCell, dColX.p, dResX.p, stream);
        nLaunch++;
        *cells = c; *cols = w;
        return KA_OK;
}

// dScore[0 .. n) to the caller: sums, and score_alignment_poar's doubles
int ka_ens_fam::scores_back(long long* sums_out, double* scores_out, int n)
{
        std::vector<unsigned long long> s((size_t)n);
        HIPCHK(hipMemcpyAsync(s.data(), dScore.p, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        nSync++;
        st[1] = evMs();
        for (int x = 0; x < n; x++) {
                const long long v = (long long)s[x];
                if (sums_out) sums_out[x] = v;
                if (scores_out) scores_out[x] = (double)v / (R > 1 ? (double)(R - 1) : 1.0);
        }
        return KA_OK;
}

int ka_ens_fam::consensus(const int* minSup, const uint8_t* letters, int nThreads)
{
        using clk = std::chrono::steady_clock;
        st[2] = st[3] = 0.0;                                     // (count, write; greedy, wall, wait, chunks, candidates, truncations)
        std::fill(st + 5, st + 11, 0.0);
        haveCons = false;
        if (ensure_maps("ka_ens_fam_consensus")) return KA_FAIL;
        // the count table of this call: levels R .. lowest, per level the rows (flat i) and E entries [i][j]
        int lowest = R + 1;
        for (int f = 0; f < F; f++) { fams[f].minSup = minSup[f]; lowest = std::min(lowest, minSup[f]); }
        const int nLev = R - lowest + 1;
        const long long ents = (long long)nLev * E, rows = (long long)nLev * S;
        if (ents > INT32_MAX) return fail("ka_ens_fam_consensus: more than 2^31 - 1 (level, i, j) counters in the batch");
        const int nRows = (int)rows;
        if (dCnt.alloc((size_t)std::max(ents, 1LL)) || dPairOff.alloc((size_t)std::max(ents, 1LL)) || dRowTot.alloc((size_t)std::max(nRows, 1)) ||
            dRowBase.alloc((size_t)std::max(nRows, 1)))
                return fail("ka_ens_fam_consensus: out of device memory (counts)");
        HIPCHK(hipMemcpyAsync(dFams.p, fams.data(), sizeof(KaEnsFam) * F, hipMemcpyHostToDevice, stream));
        KaEnsFamArgs a = args();
        a.cnt = dCnt.p; a.pairOff = dPairOff.p; a.rowBase = dRowBase.p;
        std::vector<long long> rowTot((size_t)nRows);
        HIPCHK(hipEventRecord(ev0, stream));
        HIPCHK(hipMemsetAsync(dCnt.p, 0, sizeof(int) * (size_t)std::max(ents, 1LL), stream));
        if (nLev > 0) {
                ka_ensf_launch_walk(KA_ENS_COUNT, a, nBlocks, ldsCand, stream);
                ka_ensf_launch_row_scan(a, nRows, dPairOff.p, dRowTot.p, stream);
                nLaunch += 2;
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev1, stream));
        if (nRows) HIPCHK(hipMemcpyAsync(rowTot.data(), dRowTot.p, sizeof(long long) * nRows, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        nSync++;
        st[2] = evMs();
        // chunks: levels descending, inside a level whole families in order, at most chunkCap candidates each (a family with
        // more is a chunk of its own; a family below its own lowest level has none).  famAt: the family's first candidate in its chunk
        struct Chunk { int level, f0, f1; long long total; };
        std::vector<Chunk> chunks;
        std::vector<long long> rowBase((size_t)nRows), famAt((size_t)std::max(nLev, 0) * F, 0), famN((size_t)std::max(nLev, 0) * F, 0);
        long long biggest = 0, all = 0;
        for (int lv = 0; lv < nLev; lv++) {
                int f0 = 0;
                long long run = 0;
                for (int f = 0; f < F; f++) {
                        long long t = 0;
                        for (int s = famFirst[f]; s < famFirst[f + 1]; s++) t += rowTot[(size_t)lv * S + s];
                        if (run > 0 && run + t > chunkCap) { chunks.push_back(Chunk{ R - lv, f0, f, run }); f0 = f; run = 0; }
                        famAt[(size_t)lv * F + f] = run;
                        famN[(size_t)lv * F + f] = t;
                        long long o = run;
                        for (int s = famFirst[f]; s < famFirst[f + 1]; s++) { rowBase[(size_t)lv * S + s] = o; o += rowTot[(size_t)lv * S + s]; }
                        run += t;
                        all += t;
                }
                if (run > 0) chunks.push_back(Chunk{ R - lv, f0, F, run });
        }
        for (const Chunk& c : chunks) biggest = std::max(biggest, c.total);
        st[9] = (double)all;
        if (nRows) {
                HIPCHK(hipMemcpyAsync(dRowBase.p, rowBase.data(), sizeof(long long) * nRows, hipMemcpyHostToDevice, stream));
                HIPCHK(hipStreamSynchronize(stream));            // (rowBase is read until here)
                nSync++;
        }
        if (biggest > pinnedCap) {
                for (int q = 0; q < 2; q++) {
                        if (pinned[q]) (void)hipHostFree(pinned[q]);
                        pinned[q] = nullptr;
                        pinnedCap = 0;
                        HIPCHK(hipHostMalloc((void**)&pinned[q], sizeof(int2) * (size_t)biggest));
                        if (dOut[q].alloc((size_t)biggest)) return fail("ka_ens_fam_consensus: out of device memory (candidates)");
                }
                pinnedCap = biggest;
        }
        const int nChunks = (int)chunks.size();
        auto enqueue = [&](int c) -> int {
                const int q = c & 1;
                const Chunk& ch = chunks[c];
                KaEnsFamArgs w = a;
                w.blk0 = blkFirst[ch.f0];
                w.level = ch.level;
                w.out = dOut[q].p;
                HIPCHK(hipEventRecord(wBeg[q], stream));
                ka_ensf_launch_walk(KA_ENS_WRITE, w, blkFirst[ch.f1] - blkFirst[ch.f0], ldsCand, stream);
                nLaunch++;
                HIPCHK(hipGetLastError());
                HIPCHK(hipEventRecord(wEnd[q], stream));
                HIPCHK(hipMemcpyAsync(pinned[q], dOut[q].p, sizeof(int2) * (size_t)ch.total, hipMemcpyDeviceToHost, stream));
                HIPCHK(hipEventRecord(ready[q], stream));
                return KA_OK;
        };
        // every family's union lives from its first level to its last; its columns come after the last chunk
        std::vector<KaEnsFamilyUnion> un(F);
        const auto t00 = clk::now();
        if (!ka_ens_deal(0, F, nThreads, [&](int f) {
                    const auto t0 = clk::now();
                    un[f].init(fams[f].N, lens.data() + famFirst[f]);
                    un[f].ms += ms_since(t0);
            }))
                return fail("ka_ens_fam_consensus: out of host memory in the greedy union");
        st[6] += ms_since(t00);
        if (nChunks && enqueue(0)) return KA_FAIL;
        for (int c = 0; c < nChunks; c++) {
                if (c + 1 < nChunks && enqueue(c + 1)) return KA_FAIL;
                const Chunk& ch = chunks[c];
                const auto t0 = clk::now();
                HIPCHK(hipEventSynchronize(ready[c & 1]));
                nSync++;
                st[7] += ms_since(t0);
                float wms = 0.0f;
                (void)hipEventElapsedTime(&wms, wBeg[c & 1], wEnd[c & 1]);
                st[3] += wms;
                st[8] += 1;
                const int* cand = reinterpret_cast<const int*>(pinned[c & 1]);
                const size_t lv = (size_t)(R - ch.level);
                const auto t1 = clk::now();
                if (!ka_ens_deal(ch.f0, ch.f1, nThreads, [&](int f) {
                            const auto t2 = clk::now();
                            un[f].join(cand + 2 * famAt[lv * F + f], famN[lv * F + f]);
                            un[f].ms += ms_since(t2);
                    }))
                        return fail("ka_ens_fam_consensus: out of host memory in the greedy union");
                st[6] += ms_since(t1);
        }
        cons.assign(F, FamResult());
        const auto t3 = clk::now();
        if (!ka_ens_deal(0, F, nThreads, [&](int f) {
                    const auto t2 = clk::now();
                    un[f].finish(letters + offs[famFirst[f]], cons[f].rows, &cons[f].W);
                    cons[f].truncations = un[f].uf.truncations;
                    cons[f].ms = un[f].ms + ms_since(t2);
                    un[f] = KaEnsFamilyUnion();                  // (its memory goes back as soon as the family is done)
            }))
                return fail("ka_ens_fam_consensus: out of host memory in the column order");
        st[6] += ms_since(t3);
        for (const FamResult& r : cons) { st[5] += r.ms; st[10] += (double)r.truncations; }
        haveCons = true;
        return KA_OK;
}

extern "C" int ka_ens_fam_check(int n_fam, const int* fam_first, const int* lens, const uint8_t* rows, const int* alnlens)
{
        return ens_fam_check("ka_ens_fam_check", n_fam, fam_first, lens, rows, alnlens, false);
}

extern "C" int ka_ens_fam_create(ka_ctx* ctx, int n_fam, const int* fam_first, const int* lens, int n_runs, ka_ens_fam** out)
{
        // (what needs no context first: a refused batch touches no device)
        if (n_runs < 1 || n_runs > KA_ENS_MAX_RUNS)
                return fail("ka_ens_fam_create: n_runs " + std::to_string(n_runs) + " outside 1.." + std::to_string(KA_ENS_MAX_RUNS) +
                            " (one bit per member in the reference's POAR table)");
        if (ens_fam_check_seqs("ka_ens_fam_create", n_fam, fam_first, lens)) return KA_FAIL;
        if (!ctx || !out) return fail("ka_ens_fam_create: bad arguments");
        *out = nullptr;
        std::unique_ptr<ka_ens_fam> h(new ka_ens_fam);
        if (ka_ctx_device_stream(ctx, &h->device, &h->stream)) return fail("ka_ens_fam_create: bad context");
        const int F = n_fam, S = fam_first[n_fam], R = n_runs;
        h->F = F; h->S = S; h->R = R;
        h->famFirst.assign(fam_first, fam_first + F + 1);
        h->lens.assign(lens, lens + S);
        h->offs.resize(S + 1);
        int t = 0;
        for (int s = 0; s < S; s++) { h->offs[s] = t; t += lens[s]; }
        h->offs[S] = h->T = t;
        h->fams.resize(F);
        h->blkFirst.resize(F + 1);
        long long blocks = 0;
        for (int f = 0; f < F; f++) {
                KaEnsFam& d = h->fams[f];
                d = KaEnsFam{};
                d.firstSeq = fam_first[f]; d.firstRes = h->offs[fam_first[f]];
                d.N = fam_first[f + 1] - fam_first[f];
                for (int s = 0; s < d.N; s++) d.maxlen = std::max(d.maxlen, lens[d.firstSeq + s]);
                d.nJC = (d.N + KA_ENS_JCHUNK - 1) / KA_ENS_JCHUNK;
                // the member columns of sequence i in LDS when they fit next to the three per-residue arrays (64 KiB): ka_ens::args' rule
                d.colInLds = (long long)(3 + R) * d.maxlen * 4 <= 65536;
                d.minSup = 1;
                h->ldsX = std::max(h->ldsX, (size_t)(3 * d.maxlen + (d.colInLds ? R * d.maxlen : 0)) * sizeof(int));
                h->ldsCand = std::max(h->ldsCand, (size_t)(d.colInLds ? R * d.maxlen : 0) * sizeof(int));
                d.cntFirst = h->E;
                h->E += (long long)d.N * d.N;
                h->blkFirst[f] = (int)blocks;
                blocks += (long long)d.N * d.nJC;
                if (blocks > INT32_MAX) return fail("ka_ens_fam_create: more than 2^31 - 1 workgroups in a walk over the batch");
        }
        h->blkFirst[F] = h->nBlocks = (int)blocks;
        h->added.assign(R, 0);
        h->memW.assign((size_t)R * F, 0);
        h->memCell.assign((size_t)R * (F + 1), 0);
        h->memRowOff.assign((size_t)R * F, 0);
        h->dRows.resize(R);
        const char* cc = std::getenv("KA_ENS_CHUNK");                    // candidates per chunk (tests force many chunks)
        h->chunkCap = cc && std::atoll(cc) > 0 ? std::atoll(cc) : (1ll << 22);
        HIPCHK(hipSetDevice(h->device));
        for (int b = 0; b < 2; b++) {
                HIPCHK(hipEventCreateWithFlags(&h->ready[b], hipEventDisableTiming));
                HIPCHK(hipEventCreate(&h->wBeg[b]));
                HIPCHK(hipEventCreate(&h->wEnd[b]));
        }
        HIPCHK(hipEventCreate(&h->ev0));
        HIPCHK(hipEventCreate(&h->ev1));
        if (h->dFams.alloc(F) || h->dFirstSeq.alloc(F + 1) || h->dBlkFirst.alloc(F + 1) || h->dOffs.alloc(S + 1) || h->dLens.alloc(S) ||
            h->dMemW.alloc(h->memW.size()) || h->dMemCell.alloc(h->memCell.size()) || h->dMemRowOff.alloc(h->memRowOff.size()) ||
            h->dXTab.alloc((size_t)3 * F + 2) || h->dXRowOff.alloc(F) || h->dScore.alloc((size_t)R * F) ||
            h->dSup.alloc((size_t)std::max(t, 1)) || h->dNp.alloc((size_t)std::max(t, 1)))
                return fail("ka_ens_fam_create: out of device memory");
        hipStream_t st = h->stream;
        HIPCHK(hipMemcpyAsync(h->dFams.p, h->fams.data(), sizeof(KaEnsFam) * F, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(h->dFirstSeq.p, h->famFirst.data(), sizeof(int) * (F + 1), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(h->dBlkFirst.p, h->blkFirst.data(), sizeof(int) * (F + 1), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(h->dOffs.p, h->offs.data(), sizeof(int) * (S + 1), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(h->dLens.p, h->lens.data(), sizeof(int) * S, hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
        *out = h.release();
        return KA_OK;
}

extern "C" void ka_ens_fam_destroy(ka_ens_fam* h)
{
        if (!h) return;
        (void)hipSetDevice(h->device);
        (void)hipStreamSynchronize(h->stream);
        delete h;
}

extern "C" int ka_ens_fam_add_member(ka_ens_fam* h, int k, const uint8_t* rows, const int* alnlens)
{
        if (!h || k < 0 || k >= h->R) return fail("ka_ens_fam_add_member: bad arguments");
        if (ens_fam_check("ka_ens_fam_add_member", h->F, h->famFirst.data(), h->lens.data(), rows, alnlens, false)) return KA_FAIL;
        const int F = h->F;
        std::vector<long long> rowOff(F);
        long long ro = 0;
        for (int f = 0; f < F; f++) { rowOff[f] = ro; ro += (long long)h->fams[f].N * (alnlens[f] + 1); }
        HIPCHK(hipSetDevice(h->device));
        h->begin();
        if (h->dRows[k].alloc((size_t)ro)) return fail("ka_ens_fam_add_member: out of device memory");
        HIPCHK(hipMemcpyAsync(h->dRows[k].p, rows, (size_t)ro, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        h->nSync++;
        std::copy_n(alnlens, F, h->memW.begin() + (size_t)k * F);
        std::copy(rowOff.begin(), rowOff.end(), h->memRowOff.begin() + (size_t)k * F);
        h->added[k] = 1;
        h->mapsFresh = false;
        h->haveCons = false;
        h->end(11);
        return KA_OK;
}

extern "C" int ka_ens_fam_score_members(ka_ens_fam* h, long long* sums_out, double* scores_out)
{
        if (!h) return fail("ka_ens_fam_score_members: bad arguments");
        HIPCHK(hipSetDevice(h->device));
        h->begin();
        if (h->ensure_maps("ka_ens_fam_score_members")) return KA_FAIL;
        const int F = h->F, R = h->R;
        HIPCHK(hipEventRecord(h->ev0, h->stream));
        HIPCHK(hipMemsetAsync(h->dScore.p, 0, sizeof(unsigned long long) * (size_t)R * F, h->stream));
        for (int k = 0; k < R; k++) {
                // member k as the alignment X: its maps are the walk's tables already
                KaEnsFamArgs a = h->args();
                a.colX = h->dCol.p + (long long)k * h->T; a.resX = h->dRes.p + h->resBase[k];
                a.xW = h->dMemW.p + (size_t)k * F; a.xCell = h->dMemCell.p + (size_t)k * (F + 1);
                a.score = h->dScore.p + (size_t)k * F;
                ka_ensf_launch_walk(KA_ENS_SCORE, a, h->nBlocks, h->ldsX, h->stream);
                h->nLaunch++;
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(h->ev1, h->stream));
        if (h->scores_back(sums_out, scores_out, R * F)) return KA_FAIL;
        h->end(13);
        return KA_OK;
}

extern "C" int ka_ens_fam_score(ka_ens_fam* h, const uint8_t* rows, const int* alnlens, long long* sums_out, double* scores_out)
{
        if (!h) return fail("ka_ens_fam_score: bad arguments");
        if (ens_fam_check("ka_ens_fam_score", h->F, h->famFirst.data(), h->lens.data(), rows, alnlens, true)) return KA_FAIL;
        HIPCHK(hipSetDevice(h->device));
        h->begin();
        if (h->ensure_maps("ka_ens_fam_score")) return KA_FAIL;
        KaEnsFamArgs a = h->args();
        int cells = 0, cols = 0;
        HIPCHK(hipEventRecord(h->ev0, h->stream));
        if (h->maps_x("ka_ens_fam_score", rows, alnlens, a, &cells, &cols)) return KA_FAIL;
        HIPCHK(hipMemsetAsync(h->dScore.p, 0, sizeof(unsigned long long) * (size_t)h->F, h->stream));
        a.score = h->dScore.p;
        ka_ensf_launch_walk(KA_ENS_SCORE, a, h->nBlocks, h->ldsX, h->stream);
        h->nLaunch++;
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(h->ev1, h->stream));
        if (h->scores_back(sums_out, scores_out, h->F)) return KA_FAIL;
        h->end(15);
        return KA_OK;
}

extern "C" int ka_ens_fam_consensus(ka_ens_fam* h, const int* min_support, const uint8_t* letters, int n_threads, int* alnlens_out)
{
        if (!h || !min_support || !letters) return fail("ka_ens_fam_consensus: bad arguments");
        if (n_threads < 1 || n_threads > 16) return fail("ka_ens_fam_consensus: n_threads " + std::to_string(n_threads) + " outside 1..16");
        for (int f = 0; f < h->F; f++)
                if (min_support[f] < 1)
                        return fail("ka_ens_fam_consensus: family " + std::to_string(f) + ": min_support " + std::to_string(min_support[f]) + " (>= 1 is needed)");
        HIPCHK(hipSetDevice(h->device));
        h->begin();
        const int rc = h->consensus(min_support, letters, n_threads);
        if (rc) { (void)hipStreamSynchronize(h->stream); return rc; }
        h->end(17);
        if (alnlens_out)
                for (int f = 0; f < h->F; f++) alnlens_out[f] = h->cons[f].W;
        return KA_OK;
}

extern "C" long long ka_ens_fam_rows_size(ka_ens_fam* h)
{
        if (!h || !h->haveCons) return -1;
        return packed_size(h->cons, h->famFirst.data());
}

extern "C" int ka_ens_fam_rows(ka_ens_fam* h, uint8_t* out, long long cap)
{
        if (!h || !out) return fail("ka_ens_fam_rows: bad arguments");
        if (!h->haveCons) return fail("ka_ens_fam_rows: no finished consensus on this handle");
        if (cap < packed_size(h->cons, h->famFirst.data())) return fail("ka_ens_fam_rows: the buffer is smaller than the rows (ka_ens_fam_rows_size)");
        pack_rows(h->cons, h->famFirst.data(), out);
        return KA_OK;
}

extern "C" int ka_ens_fam_confidence(ka_ens_fam* h, const uint8_t* rows, const int* alnlens, float* res_conf_out, float* col_conf_out)
{
        if (!h || !res_conf_out || !col_conf_out) return fail("ka_ens_fam_confidence: bad arguments");
        if (ens_fam_check("ka_ens_fam_confidence", h->F, h->famFirst.data(), h->lens.data(), rows, alnlens, false)) return KA_FAIL;
        HIPCHK(hipSetDevice(h->device));
        h->begin();
        if (h->ensure_maps("ka_ens_fam_confidence")) return KA_FAIL;
        KaEnsFamArgs a = h->args();
        int cells = 0, cols = 0;
        HIPCHK(hipEventRecord(h->ev0, h->stream));
        if (h->maps_x("ka_ens_fam_confidence", rows, alnlens, a, &cells, &cols)) return KA_FAIL;
        if (h->dConf.alloc((size_t)cells) || h->dColConf.alloc((size_t)cols)) return fail("ka_ens_fam_confidence: out of device memory");
        const size_t T1 = (size_t)std::max(h->T, 1);
        HIPCHK(hipMemsetAsync(h->dSup.p, 0, sizeof(int) * T1, h->stream));
        HIPCHK(hipMemsetAsync(h->dNp.p, 0, sizeof(int) * T1, h->stream));
        a.supSum = h->dSup.p; a.nPair = h->dNp.p;
        ka_ensf_launch_walk(KA_ENS_CONF, a, h->nBlocks, h->ldsX, h->stream);
        ka_ensf_launch_conf(a, cells, cols, h->dConf.p, h->dColConf.p, h->stream);
        h->nLaunch += 3;
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(h->ev1, h->stream));
        HIPCHK(hipMemcpyAsync(res_conf_out, h->dConf.p, sizeof(float) * (size_t)cells, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(col_conf_out, h->dColConf.p, sizeof(float) * (size_t)cols, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        h->nSync++;
        h->st[4] = h->evMs();
        h->end(19);
        return KA_OK;
}

extern "C" int ka_ens_fam_stats(ka_ens_fam* h, double* stats_out)
{
        if (!h) return fail("ka_ens_fam_stats: bad arguments");
        if (stats_out) std::copy_n(h->st, KA_ENS_FAM_STATS, stats_out);
        return KA_OK;
}

extern "C" int ka_debug_ens_fam_consensus_host(int n_fam, const int* fam_first, const int* lens, const long long* cand_first, const int* cand,
                                               const uint8_t* letters, int n_threads, int* alnlens_out, uint8_t* rows_out, long long cap)
{
        const std::string me = "ka_debug_ens_fam_consensus_host";
        if (!cand_first || !letters || !alnlens_out) return fail(me + ": bad arguments");
        if (n_threads < 1 || n_threads > 16) return fail(me + ": n_threads " + std::to_string(n_threads) + " outside 1..16");
        if (ens_fam_check_seqs(me, n_fam, fam_first, lens)) return KA_FAIL;
        const int S = fam_first[n_fam];
        std::vector<int> offs(S + 1, 0);
        for (int s = 0; s < S; s++) offs[s + 1] = offs[s] + lens[s];
        if (cand_first[0] != 0) return fail(me + ": cand_first does not ascend from 0");
        for (int f = 0; f < n_fam; f++) {
                if (cand_first[f + 1] < cand_first[f]) return fail(me + ": cand_first does not ascend from 0");
                if (cand_first[f + 1] > cand_first[f] && !cand) return fail(me + ": bad arguments");
                const int Tf = offs[fam_first[f + 1]] - offs[fam_first[f]];
                for (long long x = 2 * cand_first[f]; x < 2 * cand_first[f + 1]; x++)
                        if (cand[x] < 0 || cand[x] >= Tf) return fail(me + ": family " + std::to_string(f) + ": a candidate names a residue outside the family");
        }
        std::vector<FamResult> res(n_fam);
        if (!build_families(0, n_fam, n_threads, fam_first, lens, offs.data(), cand_first, cand, letters, res))
                return fail(me + ": out of host memory in the greedy union");
        for (int f = 0; f < n_fam; f++) alnlens_out[f] = res[f].W;
        if (!rows_out || cap < packed_size(res, fam_first)) return KA_ERR_ROWS_STRIDE;
        pack_rows(res, fam_first, rows_out);
        return KA_OK;
}
