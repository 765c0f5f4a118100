// ka_ens_core.h -- the host core of the ensemble consensus stage (implemented in ka_ens.cpp): the family tables, the members'
// and an alignment's maps, the stage's buffers and its sequences, each written once.  ka_ens (ka_ens.cpp, a table of one
// family) and ka_ens_fam (ka_ens_fam.cpp) are fronts over it.
#pragma once
#include <chrono>
#include <functional>
#include "ka_ctx.h"
#include "ka_ens.h"
#include "ka_msa.h"

// a front's rows to `dst` in the layout it has stated (stream-ordered); KA_OK or KA_FAIL
typedef std::function<int(uint8_t* dst, hipStream_t s)> KaEnsUpload;
// SCORE / CONF from another source of support than the members (a loaded table), with the X maps and outputs of `a`
typedef std::function<void(const KaEnsFamArgs& a)> KaEnsSupport;

// a piece of one level's candidates that crosses to the host in one copy: the front's units u0 .. u1 (rows or families), the
// walk's workgroups blk0 .. blk0 + nBlk
struct KaEnsChunk { int level, u0, u1, blk0, nBlk; long long total; };

inline double ka_ens_ms_since(std::chrono::steady_clock::time_point t0)
{
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

struct KaEnsCore {
        int device = 0;
        hipStream_t stream = nullptr;
        int F = 0, S = 0, T = 0, R = 0, nBlocks = 0;
        const char* xWho = nullptr;                              // names an allocation failure of the X maps (NULL: the call does)
        int rowPad = 0;                                          // a row of width W lies W + rowPad bytes from the next, members and X alike
        long long E = 0;                                         // entries [i][j] of one level of a count table over all rows
        long long chunkCap = 0;                                  // KA_ENS_CHUNK: candidates per chunk
        int countRows = 0;                                       // KA_ENS_COUNT_ROWS: rows of a count block of ka_ens (0: not set)
        std::vector<int> famFirst, lens, offs, blkFirst;
        std::vector<KaEnsFam> fams;
        std::vector<uint8_t> added;                              // member k was added
        std::vector<int> memW, memCell;                          // [R][F], [R][F + 1]
        std::vector<long long> memRowOff;                        // [R][F]
        std::vector<int> xTab;                                   // the tables of the last alignments X (maps_x)
        std::vector<long long> xRowOff;
        long long resBase[KA_ENS_MAX_RUNS] = {};
        bool mapsFresh = false;
        size_t ldsX = 0, ldsCand = 0;                            // the walk's LDS with and without an alignment X
        std::vector<DevBuf<uint8_t>> dRows;                      // member k's rows
        DevBuf<KaEnsFam> dFams;
        DevBuf<int> dFirstSeq, dBlkFirst, dOffs, dLens, dCol, dMemW, dMemCell, dColX, dXTab, dSup, dNp, dCnt;
        DevBuf<long long> dMemRowOff, dXRowOff, dPairOff, dRowTot, dRowBase;
        DevBuf<int16_t> dRes, dResX;
        DevBuf<uint8_t> dRowsX;
        DevBuf<unsigned long long> dScore;                       // [R][F]
        DevBuf<float> dConf, dColConf;
        DevBuf<int2> dOut[2];
        int2* pinned[2] = { nullptr, nullptr };
        long long pinnedCap = 0;
        hipEvent_t ready[2] = { nullptr, nullptr }, wBeg[2] = { nullptr, nullptr }, wEnd[2] = { nullptr, nullptr }, ev0 = nullptr, ev1 = nullptr;
        double mapsMs = 0.0, scoreMs = 0.0, confMs = 0.0;        // device time of the last sequence of each kind
        int nLaunch = 0, nSync = 0;                              // kernels launched and host waits, since the front set them to 0

        ~KaEnsCore();
        float evMs() { float m = 0.0f; (void)hipEventElapsedTime(&m, ev0, ev1); return m; }
        // The tables of n_fam families (checked by the front) of n_runs members on ctx's device.  Errors read "<who>: ...".
        int create(const char* who, ka_ctx* ctx, int n_fam, const int* fam_first, const int* lens, int n_runs, int rowPad);
        void close();                                            // waits for the stream
        KaEnsFamArgs args() const;                               // the tables; a count table over all rows
        // a member of these widths has fewer than 2^31 cells in its maps (asked before anything of member k is replaced)
        int member_fits(const char* who, int k, const int* alnlens) const;
        // member k's rows are in dRows[k], family f's alnlens[f] wide: its table entries, here and (stream-ordered) on the device
        int member_added(int k, const int* alnlens);
        int ensure_maps(const char* who);                        // one maps launch per member
        // the alignments X (alnlens[f] <= 0: none for family f): upload, their maps in dColX / dResX and their tables in a
        int maps_x(const char* who, const int* alnlens, const KaEnsUpload& upload, KaEnsFamArgs& a, int* cells, int* cols);
        // SCORE of the alignments X, one sum per family (this and the next two: after ensure_maps)
        int score_x(const char* who, const int* alnlens, const KaEnsUpload& upload, const KaEnsSupport* other, long long* sums_out, double* scores_out);
        int score_members(long long* sums_out, double* scores_out);                       // [R][F]: member k as the alignment X
        // CONF and the two confidence kernels: per cell of the X maps and per flat column
        int confidence(const char* who, const int* alnlens, const KaEnsUpload& upload, const KaEnsSupport* other, float* res_conf_out, float* col_conf_out);
        // One count table: nLev levels of a.rows rows (a.row0, a.cnt0, a.E say which).  count(a) fills a.cnt, the rows are scanned
        // into dPairOff; rowTot [nLev * a.rows] (and, when asked for, the counts themselves) come to the host.  Adds the device time to *ms.
        int count_block(const char* who, KaEnsFamArgs& a, int nLev, const std::function<void(const KaEnsFamArgs&)>& count, std::vector<long long>& rowTot,
                        std::vector<int>* pairCnt, double* ms);
        // the first slot of every row of the count table, relative to its chunk, into dRowBase (the write passes read it there);
        // oom: the front's words when the device has no memory for it
        int put_row_base(const char* oom, const std::vector<long long>& rowBase);
        // write(chunk, out) puts chunk c + 1 into the other device buffer while consume(chunk, items) takes chunk c from pinned
        // memory; a chunk without items is consumed without a write.  Adds to *writeMs (device), *waitMs (host) and *nChunks.
        int hand_over(const char* who, const std::vector<KaEnsChunk>& chunks, const std::function<void(const KaEnsChunk&, int2* out)>& write,
                      const std::function<int(const KaEnsChunk&, const int2* items)>& consume, double* writeMs, double* waitMs, double* nChunks);

private:
        int scores_back(long long* sums_out, double* scores_out, int n);
};
