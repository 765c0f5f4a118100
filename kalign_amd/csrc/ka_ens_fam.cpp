// ka_ens_fam.cpp -- host side of the ensemble consensus stage for a batch of families with the same number of members: the
// ka_ens_fam handle of the C ABI, a front over KaEnsCore (ka_ens_core.h; ka_ens.cpp holds the core and the one-family front).
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
#include "ka_ens_core.h"
#include "ka_ens_union.h"

namespace {

const char* const kWhyRes = "residue indices must stay below 4096 (the reference's POAR key ri << 20 | rj aliases beyond)";

// the families and their sequences: fam_first ascends from 0, no family is empty, every family's lengths as ka_ens_create takes them
int ens_fam_check_seqs(const std::string& me, int n_fam, const int* fam_first, const int* lens)
{
        if (!lens) return fail(me + ": bad arguments");
        if (ka_fam_check_first(me, n_fam, fam_first)) return KA_FAIL;
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
                r.ms = ka_ens_ms_since(t0);
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
        KaEnsCore core;                                          // rows W + 1 bytes apart, as ka_batch_rows packs them
        std::vector<FamResult> cons;                             // the last consensus
        bool haveCons = false;
        double st[KA_ENS_FAM_STATS] = {};

        void begin() { core.nLaunch = core.nSync = 0; }
        void end(int slot) { st[slot] = core.nLaunch; st[slot + 1] = core.nSync; st[0] = core.mapsMs; }
        // a packed batch (alnlens[f] <= 0: no rows for family f) to the device as it is
        static KaEnsUpload upload(const uint8_t* rows, const int* alnlens, KaEnsCore& c)
        {
                long long ro = 0;
                for (int f = 0; f < c.F; f++)
                        if (alnlens[f] > 0) ro += (long long)c.fams[f].N * (alnlens[f] + 1);
                int* nSync = &c.nSync;
                return [rows, ro, nSync](uint8_t* dst, hipStream_t s) {
                        if (ro) HIPCHK(hipMemcpyAsync(dst, rows, (size_t)ro, hipMemcpyHostToDevice, s));
                        HIPCHK(hipStreamSynchronize(s));         // (the caller's rows are read until here)
                        (*nSync)++;
                        return KA_OK;
                };
        }
        int consensus(const int* minSup, const uint8_t* letters, int nThreads);
};

int ka_ens_fam::consensus(const int* minSup, const uint8_t* letters, int nThreads)
{
        using clk = std::chrono::steady_clock;
        st[2] = st[3] = 0.0;                                     // (count, write; greedy, wall, wait, chunks, candidates, truncations)
        std::fill(st + 5, st + 11, 0.0);
        haveCons = false;
        const char* who = "ka_ens_fam_consensus";
        KaEnsCore& c = core;
        const int F = c.F, S = c.S, R = c.R;
        const std::vector<KaEnsFam>& fams = c.fams;
        const std::vector<int>&famFirst = c.famFirst, &lens = c.lens, &offs = c.offs;
        if (c.ensure_maps(who)) return KA_FAIL;
        // the count table of this call: levels R .. lowest, per level the rows (flat i) and E entries [i][j]
        int lowest = R + 1;
        for (int f = 0; f < F; f++) { c.fams[f].minSup = minSup[f]; lowest = std::min(lowest, minSup[f]); }
        const int nLev = R - lowest + 1;
        HIPCHK(hipMemcpyAsync(c.dFams.p, fams.data(), sizeof(KaEnsFam) * F, hipMemcpyHostToDevice, c.stream));
        KaEnsFamArgs a = c.args();
        std::vector<long long> rowTot;
        if (c.count_block(who, a, nLev, [&](const KaEnsFamArgs& g) { ka_ens_launch_walk(KA_ENS_COUNT, g, c.nBlocks, c.ldsCand, c.stream); }, rowTot, nullptr, &st[2]))
                return KA_FAIL;
        // chunks: levels descending, inside a level whole families in order, at most chunkCap candidates each (a family with
        // more is a chunk of its own; a family below its own lowest level has none).  famAt: the family's first candidate in its chunk
        std::vector<KaEnsChunk> chunks;
        std::vector<long long> rowBase(rowTot.size()), famAt((size_t)std::max(nLev, 0) * F, 0), famN((size_t)std::max(nLev, 0) * F, 0);
        long long all = 0;
        for (int lv = 0; lv < nLev; lv++) {
                int f0 = 0;
                long long run = 0;
                for (int f = 0; f < F; f++) {
                        long long t = 0;
                        for (int s = famFirst[f]; s < famFirst[f + 1]; s++) t += rowTot[(size_t)lv * S + s];
                        if (run > 0 && run + t > c.chunkCap) { chunks.push_back(KaEnsChunk{ R - lv, f0, f, c.blkFirst[f0], c.blkFirst[f] - c.blkFirst[f0], run }); f0 = f; run = 0; }
                        famAt[(size_t)lv * F + f] = run;
                        famN[(size_t)lv * F + f] = t;
                        long long o = run;
                        for (int s = famFirst[f]; s < famFirst[f + 1]; s++) { rowBase[(size_t)lv * S + s] = o; o += rowTot[(size_t)lv * S + s]; }
                        run += t;
                        all += t;
                }
                if (run > 0) chunks.push_back(KaEnsChunk{ R - lv, f0, F, c.blkFirst[f0], c.blkFirst[F] - c.blkFirst[f0], run });
        }
        st[9] = (double)all;
        if (c.put_row_base("ka_ens_fam_consensus: out of device memory (counts)", rowBase)) return KA_FAIL;
        a.rowBase = c.dRowBase.p;
        // every family's union lives from its first level to its last; its columns come after the last chunk
        std::vector<KaEnsFamilyUnion> un(F);
        const auto t00 = clk::now();
        if (!ka_ens_deal(0, F, nThreads, [&](int f) {
                    const auto t0 = clk::now();
                    un[f].init(fams[f].N, lens.data() + famFirst[f]);
                    un[f].ms += ka_ens_ms_since(t0);
            }))
                return fail("ka_ens_fam_consensus: out of host memory in the greedy union");
        st[6] += ka_ens_ms_since(t00);
        const int rc = c.hand_over(who, chunks, [&](const KaEnsChunk& ch, int2* out) {
                KaEnsFamArgs w = a;
                w.blk0 = ch.blk0; w.level = ch.level; w.out = out;
                ka_ens_launch_walk(KA_ENS_WRITE, w, ch.nBlk, c.ldsCand, c.stream);
        }, [&](const KaEnsChunk& ch, const int2* items) {
                const int* cand = reinterpret_cast<const int*>(items);
                const size_t lv = (size_t)(R - ch.level);
                const auto t1 = clk::now();
                if (!ka_ens_deal(ch.u0, ch.u1, nThreads, [&](int f) {
                            const auto t2 = clk::now();
                            un[f].join(cand + 2 * famAt[lv * F + f], famN[lv * F + f]);
                            un[f].ms += ka_ens_ms_since(t2);
                    }))
                        return fail("ka_ens_fam_consensus: out of host memory in the greedy union");
                st[6] += ka_ens_ms_since(t1);
                return KA_OK;
        }, &st[3], &st[7], &st[8]);
        if (rc) return rc;
        cons.assign(F, FamResult());
        const auto t3 = clk::now();
        if (!ka_ens_deal(0, F, nThreads, [&](int f) {
                    const auto t2 = clk::now();
                    un[f].finish(letters + offs[famFirst[f]], cons[f].rows, &cons[f].W);
                    cons[f].truncations = un[f].uf.truncations;
                    cons[f].ms = un[f].ms + ka_ens_ms_since(t2);
                    un[f] = KaEnsFamilyUnion();                  // (its memory goes back as soon as the family is done)
            }))
                return fail("ka_ens_fam_consensus: out of host memory in the column order");
        st[6] += ka_ens_ms_since(t3);
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
        if (h->core.create("ka_ens_fam_create", ctx, n_fam, fam_first, lens, n_runs, 1)) return KA_FAIL;
        *out = h.release();
        return KA_OK;
}

extern "C" void ka_ens_fam_destroy(ka_ens_fam* h)
{
        if (!h) return;
        h->core.close();
        delete h;
}

extern "C" int ka_ens_fam_add_member(ka_ens_fam* h, int k, const uint8_t* rows, const int* alnlens)
{
        if (!h || k < 0 || k >= h->core.R) return fail("ka_ens_fam_add_member: bad arguments");
        KaEnsCore& c = h->core;
        if (ens_fam_check("ka_ens_fam_add_member", c.F, c.famFirst.data(), c.lens.data(), rows, alnlens, false)) return KA_FAIL;
        const long long ro = ka_fam_row_bytes(c.F, c.famFirst.data(), alnlens);
        HIPCHK(hipSetDevice(c.device));
        h->begin();
        if (c.dRows[k].alloc((size_t)ro)) return fail("ka_ens_fam_add_member: out of device memory");
        HIPCHK(hipMemcpyAsync(c.dRows[k].p, rows, (size_t)ro, hipMemcpyHostToDevice, c.stream));
        if (c.member_added(k, alnlens)) return KA_FAIL;
        HIPCHK(hipStreamSynchronize(c.stream));
        c.nSync++;
        h->haveCons = false;
        h->end(11);
        return KA_OK;
}

extern "C" int ka_ens_fam_score_members(ka_ens_fam* h, long long* sums_out, double* scores_out)
{
        if (!h) return fail("ka_ens_fam_score_members: bad arguments");
        HIPCHK(hipSetDevice(h->core.device));
        h->begin();
        if (h->core.ensure_maps("ka_ens_fam_score_members") || h->core.score_members(sums_out, scores_out)) return KA_FAIL;
        h->st[1] = h->core.scoreMs;
        h->end(13);
        return KA_OK;
}

extern "C" int ka_ens_fam_score(ka_ens_fam* h, const uint8_t* rows, const int* alnlens, long long* sums_out, double* scores_out)
{
        if (!h) return fail("ka_ens_fam_score: bad arguments");
        KaEnsCore& c = h->core;
        if (ens_fam_check("ka_ens_fam_score", c.F, c.famFirst.data(), c.lens.data(), rows, alnlens, true)) return KA_FAIL;
        HIPCHK(hipSetDevice(c.device));
        h->begin();
        if (c.ensure_maps("ka_ens_fam_score")) return KA_FAIL;
        if (c.score_x("ka_ens_fam_score", alnlens, ka_ens_fam::upload(rows, alnlens, c), nullptr, sums_out, scores_out)) return KA_FAIL;
        h->st[1] = c.scoreMs;
        h->end(15);
        return KA_OK;
}

extern "C" int ka_ens_fam_consensus(ka_ens_fam* h, const int* min_support, const uint8_t* letters, int n_threads, int* alnlens_out)
{
        if (!h || !min_support || !letters) return fail("ka_ens_fam_consensus: bad arguments");
        if (n_threads < 1 || n_threads > 16) return fail("ka_ens_fam_consensus: n_threads " + std::to_string(n_threads) + " outside 1..16");
        for (int f = 0; f < h->core.F; f++)
                if (min_support[f] < 1)
                        return fail("ka_ens_fam_consensus: family " + std::to_string(f) + ": min_support " + std::to_string(min_support[f]) + " (>= 1 is needed)");
        HIPCHK(hipSetDevice(h->core.device));
        h->begin();
        const int rc = h->consensus(min_support, letters, n_threads);
        if (rc) { (void)hipStreamSynchronize(h->core.stream); return rc; }
        h->end(17);
        if (alnlens_out)
                for (int f = 0; f < h->core.F; f++) alnlens_out[f] = h->cons[f].W;
        return KA_OK;
}

extern "C" long long ka_ens_fam_rows_size(ka_ens_fam* h)
{
        if (!h || !h->haveCons) return -1;
        return packed_size(h->cons, h->core.famFirst.data());
}

extern "C" int ka_ens_fam_rows(ka_ens_fam* h, uint8_t* out, long long cap)
{
        if (!h || !out) return fail("ka_ens_fam_rows: bad arguments");
        if (!h->haveCons) return fail("ka_ens_fam_rows: no finished consensus on this handle");
        if (cap < packed_size(h->cons, h->core.famFirst.data())) return fail("ka_ens_fam_rows: the buffer is smaller than the rows (ka_ens_fam_rows_size)");
        pack_rows(h->cons, h->core.famFirst.data(), out);
        return KA_OK;
}

extern "C" int ka_ens_fam_confidence(ka_ens_fam* h, const uint8_t* rows, const int* alnlens, float* res_conf_out, float* col_conf_out)
{
        if (!h || !res_conf_out || !col_conf_out) return fail("ka_ens_fam_confidence: bad arguments");
        KaEnsCore& c = h->core;
        if (ens_fam_check("ka_ens_fam_confidence", c.F, c.famFirst.data(), c.lens.data(), rows, alnlens, false)) return KA_FAIL;
        HIPCHK(hipSetDevice(c.device));
        h->begin();
        if (c.ensure_maps("ka_ens_fam_confidence")) return KA_FAIL;
        if (c.confidence("ka_ens_fam_confidence", alnlens, ka_ens_fam::upload(rows, alnlens, c), nullptr, res_conf_out, col_conf_out)) return KA_FAIL;
        h->st[4] = c.confMs;
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
