// ka_cod.cpp -- host side of the codon stage: coding DNA of a batch of families, aligned in frame (include/kalign_amd.h,
// the codon stage): the ka_cod_fam handle of the C ABI, and the two functions that need no GPU (table, check).
//
// Create packs and translates on the device in two launches back to back (ka_cod.hip: cod_pack, cod_translate) and waits
// once: the host needs the records, to refuse what has no whole codons or no protein, and the proteins, which go to an
// input stage of their own (ka_in_fam_create with the biotype forced to protein) from host memory -- at most a third of the
// bytes of the DNA, and ka_in_fam_create stays as it is.  The stop-free codon plane stays on the device; a
// backtranslation (cod_back) uploads protein rows, writes the codon rows and the rows' residue counts in one launch, and
// the host checks the counts against the records before it keeps anything.
//
// -DKA_COD_HOST_ONLY builds the two host functions alone (no HIP runtime, no context): a stand-alone program can link them,
// and ka_in.cpp built with -DKA_IN_HOST_ONLY, with a fail() of its own.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#ifdef KA_COD_HOST_ONLY
#include "ka_fam.h"
#define KA_COD_LETTERS "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSS*CWCLFLF"
#else
#include <chrono>
#include <memory>
#include "ka_ctx.h"
#include "ka_cod.h"
#endif

extern "C" int ka_cod_table(uint8_t* out64)
{
        static_assert(sizeof(KA_COD_LETTERS) == 65, "64 codons");
        if (!out64) return fail("ka_cod_table: bad arguments");
        std::memcpy(out64, KA_COD_LETTERS, 64);
        return KA_OK;
}

extern "C" int ka_cod_fam_check(int n_fam, const int* fam_first, const long long* seq_off, long long n_bytes)
{
        return ka_in_check_named("ka_cod_fam_check", n_fam, fam_first, seq_off, n_bytes);
}

#ifndef KA_COD_HOST_ONLY

struct ka_cod_fam : KaStage {
        ka_ctx* ctx = nullptr;
        int nFam = 0, nSeq = 0;
        long long nBytes = 0;
        std::vector<int> famFirst;
        std::vector<int> devRecs;                        // [nSeq][KA_COD_DEVREC], input order
        std::vector<uint8_t> proteins;                   // one after the other, input order
        std::vector<long long> protOff;                  // [nSeq + 1]
        ka_in_fam* inp = nullptr;                        // the proteins' own input stage
        bool have = false;                               // a backtranslation's result is held
        std::vector<uint8_t> protRows, codRows;          // packed as ka_batch_rows packs them, input order
        std::vector<int> protLen, codLen;                // per family
        DevBuf<uint8_t> dText, dPacked, dProtein, dKept, dTable, dRows, dOut;
        DevBuf<long long> dSeqOff, dRowOff, dOutOff;
        DevBuf<int> dRecs, dFamFirst, dAlnlen, dCount;
        double st[KA_COD_STATS] = {};          // [3], [4] create's launches and waits, [5], [6] the last backtranslation's

        ~ka_cod_fam()
        {
                if (inp) ka_in_fam_destroy(inp);
        }
        int rec(int i, int k) const { return devRecs[(size_t)i * KA_COD_DEVREC + k]; }
        int nKept(int i) const { return rec(i, KA_COD_CODONS) - rec(i, KA_COD_STOPS); }
        std::string where(const std::string& me, int f, int i) const { return ka_fam_where(me, f, i - famFirst[f]); }
        int create(const std::string& me, const uint8_t* text, const long long* seq_off, const uint8_t* names, const long long* name_off);
        int back(const std::string& me, const uint8_t* rows, long long n_bytes, const int* alnlens, uint8_t gap_char);
};

int ka_cod_fam::create(const std::string& me, const uint8_t* text, const long long* seq_off, const uint8_t* names, const long long* name_off)
{
        if (open(5)) return KA_FAIL;
        begin();
        devRecs.assign((size_t)nSeq * KA_COD_DEVREC, 0);
        std::vector<uint8_t> plane((size_t)nBytes);
        if (dText.alloc((size_t)nBytes) || dPacked.alloc((size_t)nBytes) || dProtein.alloc((size_t)nBytes) || dKept.alloc((size_t)nBytes) ||
            dTable.alloc(64) || dSeqOff.alloc((size_t)nSeq + 1) || dRecs.alloc(devRecs.size()))
                return fail(me + ": out of device memory");
        uint8_t table[64];
        ka_cod_table(table);
        KaCodTab a{};
        a.nSeq = nSeq; a.text = dText.p; a.seqOff = dSeqOff.p; a.recs = dRecs.p; a.table = dTable.p;
        a.packed = dPacked.p; a.protein = dProtein.p; a.kept = dKept.p;
        if (nBytes) HIPCHK(hipMemcpyAsync(dText.p, text, (size_t)nBytes, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(dSeqOff.p, seq_off, sizeof(long long) * ((size_t)nSeq + 1), hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(dTable.p, table, sizeof table, hipMemcpyHostToDevice, stream));
        HIPCHK(hipEventRecord(ev[0], stream));
        ka_cod_run_pack(a, stream, &nLaunch);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev[1], stream));
        ka_cod_run_translate(a, stream, &nLaunch);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev[2], stream));
        HIPCHK(hipMemcpyAsync(devRecs.data(), dRecs.p, sizeof(int) * devRecs.size(), hipMemcpyDeviceToHost, stream));
        // (the plane as it lies: a sequence's protein fills at most the first third of its range, and where it ends is in the
        // records that come down with it)
        if (nBytes) HIPCHK(hipMemcpyAsync(plane.data(), dProtein.p, (size_t)nBytes, hipMemcpyDeviceToHost, stream));
        if (wait()) return KA_FAIL;
        st[0] = ms(0, 1); st[1] = ms(1, 2);
        st[3] = nLaunch; st[4] = nSync; st[7] = (double)nBytes;

        // ---- the host step: errors in batch order, then the proteins one after the other ----
        for (int f = 0; f < nFam; f++)
                for (int i = famFirst[f]; i < famFirst[f + 1]; i++) {
                        const int bad = rec(i, KA_COD_BAD);
                        if (bad < 0) continue;
                        char hex[8];
                        snprintf(hex, sizeof hex, "0x%02x", (unsigned)text[seq_off[i] + bad]);
                        return fail(where(me, f, i) + ": byte " + hex + " at offset " + std::to_string(bad));
                }
        for (int f = 0; f < nFam; f++)
                for (int i = famFirst[f]; i < famFirst[f + 1]; i++) {
                        if (rec(i, KA_COD_RESIDUES) % 3)
                                return fail(where(me, f, i) + ": " + std::to_string(rec(i, KA_COD_RESIDUES)) + " residues, not a multiple of 3");
                        if (nKept(i) <= 0) return fail(where(me, f, i) + " has no protein");
                }
        protOff.assign((size_t)nSeq + 1, 0);
        for (int i = 0; i < nSeq; i++) protOff[i + 1] = protOff[i] + nKept(i);
        proteins.resize((size_t)protOff[nSeq]);
        for (int i = 0; i < nSeq; i++) std::copy_n(&plane[(size_t)seq_off[i]], (size_t)nKept(i), &proteins[(size_t)protOff[i]]);
        // the raw text, the packed residues and the protein plane have served: a backtranslation reads the stop-free codons
        dText.release(); dPacked.release(); dProtein.release(); dTable.release();
        const std::vector<int> protein(nFam, 0);
        return ka_in_fam_create(ctx, nFam, famFirst.data(), proteins.data(), protOff.data(), names, name_off, protein.data(), &inp);
}

int ka_cod_fam::back(const std::string& me, const uint8_t* rows, long long n_bytes, const int* alnlens, uint8_t gap_char)
{
        have = false;
        std::vector<long long> rowOff(nFam), outOff(nFam);
        long long need = 0, outBytes = 0;
        for (int f = 0; f < nFam; f++) {
                if (alnlens[f] < 0) return fail(me + ": family " + std::to_string(f) + ": alignment length " + std::to_string(alnlens[f]));
                const long long N = famFirst[f + 1] - famFirst[f];
                rowOff[f] = need; outOff[f] = outBytes;
                need += N * ((long long)alnlens[f] + 1);
                outBytes += N * (3ll * alnlens[f] + 1);
        }
        if (need != n_bytes)
                return fail(me + ": " + std::to_string(n_bytes) + " bytes of rows, the alignment lengths say " + std::to_string(need));
        HIPCHK(hipSetDevice(device));
        begin();
        std::vector<int> count(nSeq, 0);
        std::vector<uint8_t> out((size_t)outBytes);
        if (dRows.alloc((size_t)need) || dOut.alloc((size_t)outBytes) || dCount.alloc(nSeq) || dFamFirst.alloc((size_t)nFam + 1) ||
            dAlnlen.alloc(nFam) || dRowOff.alloc(nFam) || dOutOff.alloc(nFam))
                return fail(me + ": out of device memory");
        KaCodBackTab a{};
        a.nFam = nFam; a.nSeq = nSeq; a.gap = gap_char; a.famFirst = dFamFirst.p; a.alnlen = dAlnlen.p; a.rowOff = dRowOff.p; a.outOff = dOutOff.p;
        a.rows = dRows.p; a.seqOff = dSeqOff.p; a.recs = dRecs.p; a.kept = dKept.p; a.out = dOut.p; a.count = dCount.p;
        HIPCHK(hipMemcpyAsync(dRows.p, rows, (size_t)need, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(dFamFirst.p, famFirst.data(), sizeof(int) * ((size_t)nFam + 1), hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(dAlnlen.p, alnlens, sizeof(int) * (size_t)nFam, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(dRowOff.p, rowOff.data(), sizeof(long long) * (size_t)nFam, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(dOutOff.p, outOff.data(), sizeof(long long) * (size_t)nFam, hipMemcpyHostToDevice, stream));
        HIPCHK(hipEventRecord(ev[3], stream));
        ka_cod_run_back(a, stream, &nLaunch);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev[4], stream));
        HIPCHK(hipMemcpyAsync(out.data(), dOut.p, (size_t)outBytes, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipMemcpyAsync(count.data(), dCount.p, sizeof(int) * (size_t)nSeq, hipMemcpyDeviceToHost, stream));
        if (wait()) return KA_FAIL;
        st[2] = ms(3, 4);
        st[5] = nLaunch; st[6] = nSync;
        for (int f = 0; f < nFam; f++)
                for (int i = famFirst[f]; i < famFirst[f + 1]; i++)
                        if (count[i] != nKept(i))
                                return fail(where(me, f, i) + ": the row holds " + std::to_string(count[i]) + " residues, the sequence " +
                                            std::to_string(nKept(i)) + " codons without stops");
        protRows.assign(rows, rows + need);
        codRows.swap(out);
        protLen.assign(alnlens, alnlens + nFam);
        codLen.resize(nFam);
        for (int f = 0; f < nFam; f++) codLen[f] = 3 * alnlens[f];
        have = true;
        return KA_OK;
}

extern "C" int ka_cod_fam_create(ka_ctx* ctx, int n_fam, const int* fam_first, const uint8_t* text, const long long* seq_off,
                                 const uint8_t* names, const long long* name_off, ka_cod_fam** out)
{
        const std::string me("ka_cod_fam_create");
        if (!ctx || !out || (names == nullptr) != (name_off == nullptr)) return fail(me + ": bad arguments");
        *out = nullptr;
        if (ka_fam_check_first(me, n_fam, fam_first)) return KA_FAIL;
        if (!seq_off) return fail(me + ": bad arguments");
        const int n = fam_first[n_fam];
        if (ka_in_check_named(me, n_fam, fam_first, seq_off, seq_off[n])) return KA_FAIL;
        if (!text && seq_off[n] > 0) return fail(me + ": bad arguments");
        if (name_off)
                for (int i = 0; i < n; i++)
                        if (name_off[i + 1] < name_off[i]) return fail(me + ": name_off does not ascend");
        std::unique_ptr<ka_cod_fam> h(new ka_cod_fam);
        if (h->attach(ctx)) return fail(me + ": bad context");
        h->ctx = ctx;
        h->nFam = n_fam; h->nSeq = n; h->nBytes = seq_off[n];
        h->famFirst.assign(fam_first, fam_first + n_fam + 1);
        if (h->create(me, text, seq_off, names, name_off)) return h->refused();
        *out = h.release();
        return KA_OK;
}

extern "C" void ka_cod_fam_destroy(ka_cod_fam* h)
{
        ka_stage_destroy(h);
}

extern "C" int ka_cod_fam_sequences(ka_cod_fam* h, int* recs_out)
{
        if (!h || !recs_out) return fail("ka_cod_fam_sequences: bad arguments");
        for (int i = 0; i < h->nSeq; i++) std::copy_n(&h->devRecs[(size_t)i * KA_COD_DEVREC], KA_COD_SEQREC, recs_out + (size_t)i * KA_COD_SEQREC);
        return KA_OK;
}

extern "C" long long ka_cod_fam_protein_size(ka_cod_fam* h)
{
        if (!h) return fail("ka_cod_fam_protein_size: bad arguments"), -1;
        return (long long)h->proteins.size();
}

extern "C" int ka_cod_fam_protein(ka_cod_fam* h, uint8_t* out, long long* off_out)
{
        if (!h) return fail("ka_cod_fam_protein: bad arguments");
        if (out) std::copy(h->proteins.begin(), h->proteins.end(), out);
        if (off_out) std::copy(h->protOff.begin(), h->protOff.end(), off_out);
        return KA_OK;
}

extern "C" int ka_cod_fam_run(ka_cod_fam* h, const float* subm, const float* scal, int n_anchors, float weight, int realign_iterations,
                              int n_threads, int refine_mode, uint8_t gap_char)
{
        if (!h || !subm || !scal) return fail("ka_cod_fam_run: bad arguments");
        const auto t0 = std::chrono::steady_clock::now();
        h->have = false;
        // (the input stage's and the batch's own messages stand)
        if (ka_in_fam_run(h->inp, 0, subm, scal, n_anchors, weight, realign_iterations, n_threads, refine_mode, gap_char)) return KA_FAIL;
        const long long need = ka_in_fam_rows_size(h->inp);
        if (need < 0) return KA_FAIL;
        std::vector<uint8_t> rows((size_t)need);
        std::vector<int> alnlens(h->nFam, 0);
        if (ka_in_fam_rows(h->inp, rows.data(), need, alnlens.data())) return KA_FAIL;
        if (h->back("ka_cod_fam_run", rows.data(), need, alnlens.data(), gap_char)) return KA_FAIL;
        h->st[8] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return KA_OK;
}

extern "C" int ka_cod_fam_back(ka_cod_fam* h, const uint8_t* protein_rows, long long n_bytes, const int* alnlens, uint8_t gap_char)
{
        if (!h || !alnlens || n_bytes < 0 || (!protein_rows && n_bytes > 0)) return fail("ka_cod_fam_back: bad arguments");
        return h->back("ka_cod_fam_back", protein_rows, n_bytes, alnlens, gap_char);
}

static long long cod_rows_size(const char* who, ka_cod_fam* h, bool protein)
{
        if (!h) return fail(std::string(who) + ": bad arguments"), -1;
        if (!h->have) return fail(std::string(who) + ": nothing has been backtranslated"), -1;
        return (long long)(protein ? h->protRows : h->codRows).size();
}

static int cod_rows(const char* who, ka_cod_fam* h, bool protein, uint8_t* out, long long cap, int* alnlens_out)
{
        if (!h || !out) return fail(std::string(who) + ": bad arguments");
        const long long need = cod_rows_size(who, h, protein);
        if (need < 0) return KA_FAIL;
        if (cap < need) return fail(std::string(who) + ": " + std::to_string(cap) + " bytes do not hold the rows (" + std::to_string(need) + ")");
        const std::vector<uint8_t>& r = protein ? h->protRows : h->codRows;
        const std::vector<int>& w = protein ? h->protLen : h->codLen;
        std::copy(r.begin(), r.end(), out);
        if (alnlens_out) std::copy(w.begin(), w.end(), alnlens_out);
        return KA_OK;
}

extern "C" long long ka_cod_fam_rows_size(ka_cod_fam* h) { return cod_rows_size("ka_cod_fam_rows_size", h, false); }

extern "C" int ka_cod_fam_rows(ka_cod_fam* h, uint8_t* out, long long cap, int* alnlens_out)
{
        return cod_rows("ka_cod_fam_rows", h, false, out, cap, alnlens_out);
}

extern "C" long long ka_cod_fam_protein_rows_size(ka_cod_fam* h) { return cod_rows_size("ka_cod_fam_protein_rows_size", h, true); }

extern "C" int ka_cod_fam_protein_rows(ka_cod_fam* h, uint8_t* out, long long cap, int* alnlens_out)
{
        return cod_rows("ka_cod_fam_protein_rows", h, true, out, cap, alnlens_out);
}

extern "C" int ka_cod_fam_stats(ka_cod_fam* h, double* out)
{
        if (!h) return fail("ka_cod_fam_stats: bad arguments");
        if (out) std::copy_n(h->st, KA_COD_STATS, out);
        return KA_OK;
}

#endif // KA_COD_HOST_ONLY
