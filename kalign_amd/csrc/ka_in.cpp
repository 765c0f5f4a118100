// ka_in.cpp -- host side of the input stage: a batch of families from raw text to the three encodings and on to rows in
// the caller's order (include/kalign_amd.h, the input stage): the ka_in_fam handle of the C ABI, and the four functions
// that need no GPU (tables, detection, order, check).
//
// The device returns exact integers per sequence and per family (ka_in.hip: in_scan); everything that decides -- the
// biotype, the aligned status, the order, the offsets -- is computed here from them, the biotype with the reference's own
// arithmetic on the same libm.  Then the second launch (in_encode) writes the three planes in sorted order, and they come
// down once: ka_in_fam_run hands them to ka_run_encoded_batch from host memory, which leaves that call as it is.
//
// -DKA_IN_HOST_ONLY builds the four host functions alone (no HIP runtime, no context): a stand-alone program can link them
// with a fail() of its own.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>
#ifdef KA_IN_HOST_ONLY
#include "ka_fam.h"
#else
#include <chrono>
#include <memory>
#include "ka_ctx.h"
#include "ka_in.h"
#endif

namespace {

constexpr int kNameLen = 256;      // MSA_NAME_LEN: names are compared over this many bytes

// ---- the three tables ----
// A table starts with the letters of an alphabet numbered in order.  A merge gives two letters the lower of their two
// codes -- one after the other, not as classes: the order of the merges is part of the result.  An alias gives a letter
// another's code as it stands at that point.  At the end the codes in use are renumbered densely in ascending order and
// lower case takes upper case's code.
struct InAlphabet {
        const char* letters;
        const char* merges;        // pairs
        const char* aliases;       // pairs: (letter, the letter whose code it takes)
        bool aliasAfter;           // aliases after the merges (else before)
};
const InAlphabet kAlphabets[3] = {
        // nucleotides: U is T, every IUPAC ambiguity code is N
        { "ACGTUNRYSWKMBDHV", "UTNRNYNSNWNKNMNBNDNHNV", "", false },
        // the reduced protein alphabet of the guide tree: (L,M) (I,V) (K,R) (E,Q) (A,S,T) (N,D) (F,Y), B with N and D, Z
        // with E and Q; selenocysteine U takes cysteine's code
        { "ACDEFGHIKLMNPQRSTVWYBZX", "LMIVKREQASATSTNDFYBNBDZEZQ", "UC", true },
        // the protein alphabet of the alignment with B, Z and X; U is X
        { "ARNDCQEGHILKMFPSTWYVBZX", "", "UX", true },
};

void build_table(const InAlphabet& a, int8_t* t)
{
        std::fill(t, t + 128, (int8_t)-1);
        for (int k = 0; a.letters[k]; k++) t[(int)a.letters[k]] = (int8_t)k;
        auto alias = [&]() { for (const char* p = a.aliases; *p; p += 2) t[(int)p[0]] = t[(int)p[1]]; };
        if (!a.aliasAfter) alias();
        for (const char* p = a.merges; *p; p += 2) t[(int)p[0]] = t[(int)p[1]] = std::min(t[(int)p[0]], t[(int)p[1]]);
        if (a.aliasAfter) alias();
        int8_t dense[32];
        bool used[32] = {};
        for (int b = 64; b < 96; b++)
                if (t[b] >= 0) used[t[b]] = true;
        int code = 0;
        for (int k = 0; k < 32; k++) dense[k] = used[k] ? (int8_t)code++ : (int8_t)-1;
        for (int b = 64; b < 96; b++)
                if (t[b] >= 0) t[b + 32] = t[b] = dense[t[b]];
}

// ---- detection ----
int detect(const std::string& me, const long long* freq, int* biotype)
{
        double dna[128], protein[128];
        for (int i = 0; i < 128; i++) {
                dna[i] = log(0.0001 * 1.0 / 116.0);
                protein[i] = log(0.0001 * 1.0 / 88.0);
        }
        for (const char* p = "acgtunACGTUN"; *p; p++) dna[(int)*p] = log(0.9999 * 1.0 / 12.0);
        for (const char* p = "acdefghiklmnpqrstvwyACDEFGHIKLMNPQRSTVWY"; *p; p++) protein[(int)*p] = log(0.9999 * 1.0 / 40.0);
        double dnaProb = 0.0, protProb = 0.0;
        for (int i = 0; i < 128; i++)
                if (freq[i]) {
                        dnaProb += dna[i] * (double)freq[i];
                        protProb += protein[i] * (double)freq[i];
                }
        if (dnaProb == protProb || std::isnan(dnaProb) || std::isnan(protProb)) return fail(me + ": could not determine the alphabet");
        *biotype = dnaProb > protProb ? 1 : 0;
        return KA_OK;
}

int in_check(const std::string& me, int n_fam, const int* fam_first, const long long* seq_off, long long n_bytes)
{
        if (ka_fam_check_first(me, n_fam, fam_first)) return KA_FAIL;
        if (!seq_off || n_bytes < 0) return fail(me + ": bad arguments");
        const int n = fam_first[n_fam];
        if (seq_off[0] != 0 || seq_off[n] != n_bytes) return fail(me + ": seq_off does not ascend from 0 to n_bytes");
        for (int f = 0; f < n_fam; f++)
                for (int i = fam_first[f]; i < fam_first[f + 1]; i++) {
                        if (seq_off[i + 1] < seq_off[i]) return fail(me + ": seq_off does not ascend from 0 to n_bytes");
                        if (seq_off[i + 1] - seq_off[i] > INT32_MAX)
                                return fail(ka_fam_where(me, f, i - fam_first[f]) + ": " + std::to_string(seq_off[i + 1] - seq_off[i]) +
                                            " bytes; a sequence holds fewer than 2^31");
                }
        return KA_OK;
}

// strncmp over kNameLen bytes of two names given by their bytes: a name ends at its length or at a 0 byte
int name_cmp(const uint8_t* a, long long la, const uint8_t* b, long long lb)
{
        for (int k = 0; k < kNameLen; k++) {
                const int x = k < la ? a[k] : 0, y = k < lb ? b[k] : 0;
                if (x != y) return x < y ? -1 : 1;
                if (!x) return 0;
        }
        return 0;
}

// more residues first, then the lower name, then the lower input index (a stable sort: equal keys keep input order)
void in_order(int n_fam, const int* fam_first, const int* residues, const uint8_t* names, const long long* name_off, int* order)
{
        const bool named = names && name_off;
        for (int i = 0; i < fam_first[n_fam]; i++) order[i] = i;
        for (int f = 0; f < n_fam; f++)
                std::stable_sort(order + fam_first[f], order + fam_first[f + 1], [&](int x, int y) {
                        if (residues[x] != residues[y]) return residues[x] > residues[y];
                        if (!named) return false;
                        return name_cmp(names + name_off[x], name_off[x + 1] - name_off[x], names + name_off[y], name_off[y + 1] - name_off[y]) < 0;
                });
}

} // namespace

extern "C" int ka_in_tables(int8_t* out3x128)
{
        if (!out3x128) return fail("ka_in_tables: bad arguments");
        for (int k = 0; k < 3; k++) build_table(kAlphabets[k], out3x128 + 128 * k);
        return KA_OK;
}

extern "C" int ka_in_detect(const long long* freq128, int* biotype_out)
{
        if (!freq128 || !biotype_out) return fail("ka_in_detect: bad arguments");
        return detect("ka_in_detect", freq128, biotype_out);
}

extern "C" int ka_in_order(int n_fam, const int* fam_first, const int* residues, const uint8_t* names, const long long* name_off, int* order_out)
{
        if (ka_fam_check_first("ka_in_order", n_fam, fam_first)) return KA_FAIL;
        if (!residues || !order_out || (names == nullptr) != (name_off == nullptr)) return fail("ka_in_order: bad arguments");
        if (name_off)
                for (int i = 0; i < fam_first[n_fam]; i++)
                        if (name_off[i + 1] < name_off[i]) return fail("ka_in_order: name_off does not ascend");
        in_order(n_fam, fam_first, residues, names, name_off, order_out);
        return KA_OK;
}

extern "C" int ka_in_fam_check(int n_fam, const int* fam_first, const long long* seq_off, long long n_bytes)
{
        return in_check("ka_in_fam_check", n_fam, fam_first, seq_off, n_bytes);
}

// the check under another stage's name (ka_fam.h: the codon stage)
int ka_in_check_named(const std::string& me, int n_fam, const int* fam_first, const long long* seq_off, long long n_bytes)
{
        return in_check(me, n_fam, fam_first, seq_off, n_bytes);
}

#ifndef KA_IN_HOST_ONLY

struct ka_in_fam : KaStage {
        ka_ctx* ctx = nullptr;
        int nFam = 0, nSeq = 0;
        long long nBytes = 0, size = 0;        // raw bytes; residues
        std::vector<int> famFirst, order, lens;          // lens[p]: residues of sorted position p
        std::vector<long long> outOff;                   // [nSeq + 1] by sorted position
        std::vector<int> seqRecs;                        // [nSeq][KA_IN_SEQREC], input order
        std::vector<int> famRecs;                        // [nFam][KA_IN_FAMREC]
        std::vector<long long> freq;                     // [nFam][KA_IN_BINS]
        std::vector<uint8_t> letters, treeCodes, codes;  // the planes, sorted order
        std::vector<std::vector<uint8_t>> rows;          // per family: its rows in input order, alnlen + 1 bytes apart
        std::vector<int> alnlen;                         // per family, -1: not run
        DevBuf<uint8_t> dText, dBiotype, dLetters, dTree, dCodes;
        DevBuf<long long> dSeqOff, dOutOff;
        DevBuf<int> dFamFirst, dRecs, dOrder;
        DevBuf<unsigned long long> dFreq, dNoCode;
        DevBuf<int8_t> dTables;
        double st[KA_IN_STATS] = {};

        int create(const std::string& me, const uint8_t* text, const long long* seq_off, const uint8_t* names, const long long* name_off,
                   const int* biotype_in);
        int run(const std::string& me, int biotype, const float* subm, const float* scal, int n_anchors, float weight, int realign_iterations,
                int n_threads, int refine_mode, uint8_t gap_char);
        int missing() const                    // the first family not yet run, or -1
        {
                for (int f = 0; f < nFam; f++)
                        if (alnlen[f] < 0) return f;
                return -1;
        }
};

int ka_in_fam::create(const std::string& me, const uint8_t* text, const long long* seq_off, const uint8_t* names, const long long* name_off,
                      const int* biotype_in)
{
        if (open(4)) return KA_FAIL;
        std::vector<int> devRecs((size_t)nSeq * KA_IN_DEVREC, 0);
        std::vector<unsigned long long> noCode(nFam, 0);
        freq.assign((size_t)nFam * KA_IN_BINS, 0);
        if (dText.alloc((size_t)nBytes) || dSeqOff.alloc((size_t)nSeq + 1) || dFamFirst.alloc((size_t)nFam + 1) || dRecs.alloc(devRecs.size()) ||
            dFreq.alloc(freq.size()) || dNoCode.alloc(nFam) || dOrder.alloc(nSeq) || dOutOff.alloc((size_t)nSeq + 1) || dBiotype.alloc(nFam) ||
            dTables.alloc(KA_IN_TABLES * 128))
                return fail(me + ": out of device memory");
        KaInTab a{};
        a.nFam = nFam; a.nSeq = nSeq; a.famFirst = dFamFirst.p; a.text = dText.p; a.seqOff = dSeqOff.p; a.recs = dRecs.p; a.freq = dFreq.p;
        if (nBytes) HIPCHK(hipMemcpyAsync(dText.p, text, (size_t)nBytes, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(dSeqOff.p, seq_off, sizeof(long long) * ((size_t)nSeq + 1), hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(dFamFirst.p, famFirst.data(), sizeof(int) * ((size_t)nFam + 1), hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemsetAsync(dFreq.p, 0, sizeof(unsigned long long) * freq.size(), stream));
        HIPCHK(hipMemsetAsync(dNoCode.p, 0, sizeof(unsigned long long) * nFam, stream));
        HIPCHK(hipEventRecord(ev[0], stream));
        ka_in_run_scan(a, stream, &nLaunch);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev[1], stream));
        HIPCHK(hipMemcpyAsync(devRecs.data(), dRecs.p, sizeof(int) * devRecs.size(), hipMemcpyDeviceToHost, stream));
        static_assert(sizeof(long long) == sizeof(unsigned long long), "the histogram comes down as it is");
        HIPCHK(hipMemcpyAsync(freq.data(), dFreq.p, sizeof(long long) * freq.size(), hipMemcpyDeviceToHost, stream));
        if (wait()) return KA_FAIL;

        // ---- the host step: errors, biotype, status, order, offsets ----
        auto where = [&](int f, int i) { return ka_fam_where(me, f, i - famFirst[f]); };
        for (int f = 0; f < nFam; f++)
                for (int i = famFirst[f]; i < famFirst[f + 1]; i++) {
                        const int bad = devRecs[(size_t)i * KA_IN_DEVREC + KA_IN_BAD];
                        if (bad < 0) continue;
                        char hex[8];
                        snprintf(hex, sizeof hex, "0x%02x", (unsigned)text[seq_off[i] + bad]);
                        return fail(where(f, i) + ": byte " + hex + " at offset " + std::to_string(bad));
                }
        for (int f = 0; f < nFam; f++)
                for (int i = famFirst[f]; i < famFirst[f + 1]; i++)
                        if (devRecs[(size_t)i * KA_IN_DEVREC + KA_IN_RESIDUES] == 0) return fail(where(f, i) + " has no residue");
        seqRecs.resize((size_t)nSeq * KA_IN_SEQREC);
        std::vector<int> residues(nSeq);
        for (int i = 0; i < nSeq; i++) {
                std::copy_n(&devRecs[(size_t)i * KA_IN_DEVREC], KA_IN_SEQREC, &seqRecs[(size_t)i * KA_IN_SEQREC]);
                residues[i] = devRecs[(size_t)i * KA_IN_DEVREC + KA_IN_RESIDUES];
        }
        famRecs.assign((size_t)nFam * KA_IN_FAMREC, 0);
        std::vector<uint8_t> biotype(nFam);
        for (int f = 0; f < nFam; f++) {
                int* r = &famRecs[(size_t)f * KA_IN_FAMREC];
                if (biotype_in && biotype_in[f] >= 0) r[0] = biotype_in[f];
                else if (detect(me + ": family " + std::to_string(f), &freq[(size_t)f * KA_IN_BINS], &r[0])) return KA_FAIL;
                biotype[f] = (uint8_t)r[0];
                // detect_aligned: residues + gap characters per sequence, and whether the family holds a gap character at all
                long long gaps = 0, minTotal = INT64_MAX, maxTotal = 0;
                int minLen = INT32_MAX, maxLen = 0;
                for (int i = famFirst[f]; i < famFirst[f + 1]; i++) {
                        const long long g = devRecs[(size_t)i * KA_IN_DEVREC + KA_IN_GAPS], total = g + residues[i];
                        gaps += g;
                        minTotal = std::min(minTotal, total); maxTotal = std::max(maxTotal, total);
                        minLen = std::min(minLen, residues[i]); maxLen = std::max(maxLen, residues[i]);
                }
                r[1] = gaps ? (minTotal == maxTotal ? 2 : 3) : (minTotal == maxTotal ? 3 : 1);
                r[2] = minLen; r[3] = maxLen;
        }
        order.resize(nSeq);
        in_order(nFam, famFirst.data(), residues.data(), names, name_off, order.data());
        outOff.assign((size_t)nSeq + 1, 0);
        lens.resize(nSeq);
        for (int p = 0; p < nSeq; p++) {
                lens[p] = residues[order[p]];
                outOff[p + 1] = outOff[p] + lens[p];
        }
        size = outOff[nSeq];
        int8_t tables[KA_IN_TABLES * 128];
        ka_in_tables(tables);

        // ---- the encode ----
        if (dLetters.alloc((size_t)size) || dTree.alloc((size_t)size) || dCodes.alloc((size_t)size)) return fail(me + ": out of device memory");
        letters.resize((size_t)size); treeCodes.resize((size_t)size); codes.resize((size_t)size);
        a.order = dOrder.p; a.outOff = dOutOff.p; a.biotype = dBiotype.p; a.tables = dTables.p;
        a.letters = dLetters.p; a.treeCodes = dTree.p; a.codes = dCodes.p; a.noCode = dNoCode.p;
        HIPCHK(hipMemcpyAsync(dOrder.p, order.data(), sizeof(int) * (size_t)nSeq, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(dOutOff.p, outOff.data(), sizeof(long long) * outOff.size(), hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(dBiotype.p, biotype.data(), (size_t)nFam, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(dTables.p, tables, sizeof tables, hipMemcpyHostToDevice, stream));
        HIPCHK(hipEventRecord(ev[2], stream));
        ka_in_run_encode(a, stream, &nLaunch);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev[3], stream));
        HIPCHK(hipMemcpyAsync(letters.data(), dLetters.p, (size_t)size, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipMemcpyAsync(treeCodes.data(), dTree.p, (size_t)size, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipMemcpyAsync(codes.data(), dCodes.p, (size_t)size, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipMemcpyAsync(noCode.data(), dNoCode.p, sizeof(unsigned long long) * nFam, hipMemcpyDeviceToHost, stream));
        if (wait()) return KA_FAIL;
        for (int f = 0; f < nFam; f++) famRecs[(size_t)f * KA_IN_FAMREC + 4] = (int)std::min<unsigned long long>(noCode[f], INT32_MAX);
        st[0] = ms(0, 1); st[1] = ms(2, 3);
        st[4] = (double)nBytes;
        // the raw text has served: the planes are what every later call reads
        dText.release();
        rows.assign(nFam, {});
        alnlen.assign(nFam, -1);
        return KA_OK;
}

// The families of one biotype, in order, as one batch: their ranges of the three planes one after the other (a family's
// sorted positions are contiguous, so each is one copy), ka_run_encoded_batch on the handle's context, and the packed rows
// back, each family's put from sorted into input order.
int ka_in_fam::run(const std::string& me, int biotype, const float* subm, const float* scal, int n_anchors, float weight, int realign_iterations,
                   int n_threads, int refine_mode, uint8_t gap_char)
{
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<int> pick;
        for (int f = 0; f < nFam; f++)
                if (famRecs[(size_t)f * KA_IN_FAMREC] == biotype) pick.push_back(f);
        if (pick.empty()) return KA_OK;
        std::vector<int> first(pick.size() + 1, 0), off, ln;
        std::vector<uint8_t> t, c, l;
        for (size_t k = 0; k < pick.size(); k++) {
                const int f = pick[k], p0 = famFirst[f], p1 = famFirst[f + 1];
                first[k + 1] = first[k] + (p1 - p0);
                if ((long long)t.size() + outOff[p1] - outOff[p0] > INT32_MAX)
                        return fail(me + ": the families of biotype " + std::to_string(biotype) + " hold 2^31 residues or more");
                for (int p = p0; p < p1; p++) {
                        off.push_back((int)(t.size() + (size_t)(outOff[p] - outOff[p0])));
                        ln.push_back(lens[p]);
                }
                t.insert(t.end(), treeCodes.begin() + outOff[p0], treeCodes.begin() + outOff[p1]);
                c.insert(c.end(), codes.begin() + outOff[p0], codes.begin() + outOff[p1]);
                l.insert(l.end(), letters.begin() + outOff[p0], letters.begin() + outOff[p1]);
        }
        const int n = first[pick.size()];
        std::vector<int> alen(n, 0);
        if (ka_run_encoded_batch(ctx, (int)pick.size(), first.data(), t.data(), c.data(), l.data(), off.data(), ln.data(), subm, scal, n_anchors,
                                 weight, realign_iterations, nullptr, n_threads, refine_mode, gap_char, alen.data()))
                return KA_FAIL;                                  // (its own message stands)
        const long long need = ka_batch_rows_size(ctx);
        if (need < 0) return fail(me + ": the batch left no rows");
        std::vector<uint8_t> packed((size_t)need);
        if (ka_batch_rows(ctx, packed.data(), need)) return KA_FAIL;
        long long at = 0;
        for (size_t k = 0; k < pick.size(); k++) {
                const int f = pick[k], p0 = famFirst[f], N = famFirst[f + 1] - p0;
                const long long W1 = (long long)alen[first[k]] + 1;
                if (at + N * W1 > need) return fail(me + ": the batch's rows are shorter than its alignment lengths say");
                std::vector<uint8_t>& r = rows[f];
                r.resize((size_t)(N * W1));
                for (int p = 0; p < N; p++)
                        std::copy_n(&packed[(size_t)(at + p * W1)], (size_t)W1, &r[(size_t)((order[p0 + p] - p0) * W1)]);
                alnlen[f] = (int)(W1 - 1);
                at += N * W1;
        }
        st[5] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return KA_OK;
}

extern "C" int ka_in_fam_create(ka_ctx* ctx, int n_fam, const int* fam_first, const uint8_t* text, const long long* seq_off,
                                const uint8_t* names, const long long* name_off, const int* biotype_in, ka_in_fam** out)
{
        const std::string me("ka_in_fam_create");
        if (!ctx || !out || (names == nullptr) != (name_off == nullptr)) return fail(me + ": bad arguments");
        *out = nullptr;
        if (ka_fam_check_first(me, n_fam, fam_first)) return KA_FAIL;
        if (!seq_off) return fail(me + ": bad arguments");
        const int n = fam_first[n_fam];
        if (in_check(me, n_fam, fam_first, seq_off, seq_off[n])) return KA_FAIL;
        if (!text && seq_off[n] > 0) return fail(me + ": bad arguments");
        if (name_off)
                for (int i = 0; i < n; i++)
                        if (name_off[i + 1] < name_off[i]) return fail(me + ": name_off does not ascend");
        if (biotype_in)
                for (int f = 0; f < n_fam; f++)
                        if (biotype_in[f] < -1 || biotype_in[f] > 1)
                                return fail(me + ": family " + std::to_string(f) + ": biotype " + std::to_string(biotype_in[f]) + " is not -1, 0 or 1");
        std::unique_ptr<ka_in_fam> h(new ka_in_fam);
        if (h->attach(ctx)) return fail(me + ": bad context");
        h->ctx = ctx;
        h->nFam = n_fam; h->nSeq = n; h->nBytes = seq_off[n];
        h->famFirst.assign(fam_first, fam_first + n_fam + 1);
        if (h->create(me, text, seq_off, names, name_off, biotype_in)) return h->refused();
        h->st[2] = h->nLaunch; h->st[3] = h->nSync;
        *out = h.release();
        return KA_OK;
}

extern "C" void ka_in_fam_destroy(ka_in_fam* h)
{
        ka_stage_destroy(h);
}

extern "C" int ka_in_fam_sequences(ka_in_fam* h, int* recs_out)
{
        if (!h || !recs_out) return fail("ka_in_fam_sequences: bad arguments");
        std::copy(h->seqRecs.begin(), h->seqRecs.end(), recs_out);
        return KA_OK;
}

extern "C" int ka_in_fam_families(ka_in_fam* h, int* recs_out, long long* freq_out)
{
        if (!h || !recs_out) return fail("ka_in_fam_families: bad arguments");
        std::copy(h->famRecs.begin(), h->famRecs.end(), recs_out);
        if (freq_out) std::copy(h->freq.begin(), h->freq.end(), freq_out);
        return KA_OK;
}

extern "C" int ka_in_fam_order(ka_in_fam* h, int* order_out)
{
        if (!h || !order_out) return fail("ka_in_fam_order: bad arguments");
        std::copy(h->order.begin(), h->order.end(), order_out);
        return KA_OK;
}

extern "C" long long ka_in_fam_size(ka_in_fam* h)
{
        if (!h) return fail("ka_in_fam_size: bad arguments"), -1;
        return h->size;
}

extern "C" int ka_in_fam_encoded(ka_in_fam* h, uint8_t* tree_codes, uint8_t* codes, uint8_t* letters, int* off, int* lens)
{
        if (!h) return fail("ka_in_fam_encoded: bad arguments");
        if (h->size > INT32_MAX) return fail("ka_in_fam_encoded: the batch holds " + std::to_string(h->size) + " residues; int offsets reach fewer than 2^31");
        if (tree_codes) std::copy(h->treeCodes.begin(), h->treeCodes.end(), tree_codes);
        if (codes) std::copy(h->codes.begin(), h->codes.end(), codes);
        if (letters) std::copy(h->letters.begin(), h->letters.end(), letters);
        if (off)
                for (int p = 0; p < h->nSeq; p++) off[p] = (int)h->outOff[p];
        if (lens) std::copy(h->lens.begin(), h->lens.end(), lens);
        return KA_OK;
}

extern "C" int ka_in_fam_run(ka_in_fam* h, int biotype, const float* subm, const float* scal, int n_anchors, float weight,
                             int realign_iterations, int n_threads, int refine_mode, uint8_t gap_char)
{
        if (!h || !subm || !scal) return fail("ka_in_fam_run: bad arguments");
        if (biotype != 0 && biotype != 1) return fail("ka_in_fam_run: biotype " + std::to_string(biotype) + " is not 0 (protein) or 1 (DNA)");
        return h->run("ka_in_fam_run", biotype, subm, scal, n_anchors, weight, realign_iterations, n_threads, refine_mode, gap_char);
}

static int in_missing(const char* who, ka_in_fam* h)
{
        const int f = h->missing();
        if (f < 0) return KA_OK;
        return fail(std::string(who) + ": family " + std::to_string(f) + " has not been run (ka_in_fam_run with biotype " +
                    std::to_string(h->famRecs[(size_t)f * KA_IN_FAMREC]) + ")");
}

extern "C" long long ka_in_fam_rows_size(ka_in_fam* h)
{
        if (!h) return fail("ka_in_fam_rows_size: bad arguments"), -1;
        if (in_missing("ka_in_fam_rows_size", h)) return -1;
        long long n = 0;
        for (const auto& r : h->rows) n += (long long)r.size();
        return n;
}

extern "C" int ka_in_fam_rows(ka_in_fam* h, uint8_t* out, long long cap, int* alnlens_out)
{
        if (!h || !out) return fail("ka_in_fam_rows: bad arguments");
        if (in_missing("ka_in_fam_rows", h)) return KA_FAIL;
        const long long need = ka_in_fam_rows_size(h);
        if (cap < need) return fail("ka_in_fam_rows: " + std::to_string(cap) + " bytes do not hold the rows (" + std::to_string(need) + ")");
        for (const auto& r : h->rows) out = std::copy(r.begin(), r.end(), out);
        if (alnlens_out) std::copy(h->alnlen.begin(), h->alnlen.end(), alnlens_out);
        return KA_OK;
}

extern "C" int ka_in_fam_stats(ka_in_fam* h, double* out)
{
        if (!h) return fail("ka_in_fam_stats: bad arguments");
        if (out) std::copy_n(h->st, KA_IN_STATS, out);
        return KA_OK;
}

#endif // KA_IN_HOST_ONLY
