// ka_out.cpp -- host side of the output stage: the finished rows of a batch of families as FASTA, Clustal, MSF and Stockholm
// text (include/kalign_amd.h, the output stage): the ka_out_fam handle of the C ABI, and the three functions that need no GPU
// (ka_out_fam_check, ka_out_fam_text_sizes, ka_out_pp_char).  One alignment is a batch of one.
//
// Rows and names go up once, at create.  A call computes where every family's text starts -- closed forms over N, W and the
// name lengths (out_layout) -- refuses a cap below the size before anything is launched, uploads the call's small tables
// (one record per family, the offsets, the headers) and launches out_fill once; text and offender record come down behind
// it and the host waits once.  MSF needs each row's characters and prefix checksum first: the row pass (out_rows) runs once
// per handle, its records stay on the host, and the MSF headers are formatted here from them with the reference's own
// format strings.  The library never reads the clock: the date is the caller's.
//
// Every check runs on the host before anything is launched: a refused call launches nothing and leaves the handle usable.
#include <cstdio>
#include <memory>
#include "ka_ctx.h"
#include "ka_out.h"

namespace {

// What the reference's CLI writes after a run, for a protein (0) and for a DNA (1) family alike: write_msa_msf tests msa->L
// against ALPHA_defPROTEIN and ALPHA_redPROTEIN, and after a run it holds neither (tests/golden/out_*.npz record both lines).
const char* const kMsfBanner[2] = { "!!NA_MULTIPLE_ALIGNMENT 1.0", "!!NA_MULTIPLE_ALIGNMENT 1.0" };
const char kMsfType[2] = { 'N', 'N' };
const char kStockholm[] = "# STOCKHOLM 1.0\n";

bool printable(int b) { return b >= 32 && b <= 126; }

int names_check(const std::string& me, int n_fam, const int* fam_first, const uint8_t* names, const long long* name_off)
{
        if ((names == nullptr) != (name_off == nullptr)) return fail(me + ": bad arguments");
        if (!names) return KA_OK;
        for (int i = 0; i < fam_first[n_fam]; i++)
                if (name_off[i + 1] < name_off[i]) return fail(me + ": name_off does not ascend");
        for (int f = 0; f < n_fam; f++)
                for (int i = fam_first[f]; i < fam_first[f + 1]; i++) {
                        const std::string at = ka_fam_where(me, f, i - fam_first[f]);
                        const long long n = name_off[i + 1] - name_off[i];
                        if (n == 0) return fail(at + ": empty name");
                        if (n > KA_OUT_NAME_MAX) return fail(at + ": name of " + std::to_string(n) + " bytes; a name holds 1 to 255");
                        for (long long k = 0; k < n; k++) {
                                const int b = names[name_off[i] + k];
                                if (printable(b)) continue;
                                char hex[8];
                                snprintf(hex, sizeof hex, "0x%02x", (unsigned)b);
                                return fail(at + ": name byte " + hex + " at offset " + std::to_string(k) + "; a name is printable ASCII (32..126)");
                        }
                }
        return KA_OK;
}

int out_check(const std::string& me, int n_fam, const int* fam_first, const uint8_t* rows, const int* alnlens, const uint8_t* names,
              const long long* name_off)
{
        if (ka_sum_check_named(me, n_fam, fam_first, rows, alnlens)) return KA_FAIL;
        return names_check(me, n_fam, fam_first, names, name_off);
}

// a string of printable ASCII, 1 .. max bytes
int text_check(const std::string& me, const std::string& what, const uint8_t* s, long long n, long long max)
{
        if (n < 1 || n > max) return fail(me + ": " + what + " of " + std::to_string(n) + " bytes; it holds 1 to " + std::to_string(max));
        for (long long k = 0; k < n; k++)
                if (!printable(s[k])) return fail(me + ": " + what + " holds a byte that is not printable ASCII (32..126)");
        return KA_OK;
}

// the families' records from the batch as given, and every row's name: as given, or "seq0", "seq1", ... per family
// (python-kalign's default); names_in NULL with name_off given: the lengths alone (the sizes need no more)
void out_families(int n_fam, const int* fam_first, const int* alnlens, const uint8_t* names_in, const long long* name_off, std::vector<KaOutFam>& fams,
                  std::vector<uint8_t>& names, std::vector<long long>& nameOff, long long* bytes, long long* cells, long long* cols)
{
        fams.assign(n_fam, KaOutFam{});
        nameOff.assign((size_t)fam_first[n_fam] + 1, 0);
        *bytes = *cells = *cols = 0;
        for (int f = 0; f < n_fam; f++) {
                KaOutFam& d = fams[f];
                d.N = fam_first[f + 1] - fam_first[f]; d.W = alnlens[f]; d.firstRow = fam_first[f]; d.rowOff = *bytes;
                d.confOff = *cells; d.colOff = *cols; d.keyBase = *cells + *cols;
                *bytes += (long long)d.N * ((long long)d.W + 1);
                *cells += (long long)d.N * d.W;
                *cols += d.W;
                for (int i = 0; i < d.N; i++) {
                        const int r = d.firstRow + i;
                        if (names_in) names.insert(names.end(), names_in + name_off[r], names_in + name_off[r + 1]);
                        else if (name_off) names.resize(names.size() + (size_t)(name_off[r + 1] - name_off[r]), (uint8_t)'?');
                        else {
                                const std::string s = "seq" + std::to_string(i);
                                names.insert(names.end(), s.begin(), s.end());
                        }
                        nameOff[r + 1] = (long long)names.size();
                        d.nameMax = std::max(d.nameMax, (int)(nameOff[r + 1] - nameOff[r]));
                }
        }
}

// Where every family's text starts (famOff [n_fam + 1]; FASTA: rowOut [numseq + 1], where a row's starts) from the families'
// records with the call's header lengths filled in; the size.  The closed forms of the three block shapes live here and in
// ka_out.h alone.
long long out_layout(const std::vector<KaOutFam>& fams, const std::vector<long long>& nameOff, int format, int lineLength, bool hasRes, bool hasCol,
                     std::vector<long long>& famOff, std::vector<long long>& rowOut)
{
        const int nFam = (int)fams.size();
        famOff.assign((size_t)nFam + 1, 0);
        if (format == KA_OUT_FASTA) rowOut.assign(nameOff.size(), 0);
        long long at = 0;
        for (int f = 0; f < nFam; f++) {
                const KaOutFam& d = fams[f];
                famOff[f] = at;
                at += d.hdrLen;
                if (format == KA_OUT_FASTA) {
                        const long long L = lineLength, body = (long long)d.W + ((long long)d.W + L - 1) / L;
                        for (int r = d.firstRow; r < d.firstRow + d.N; r++) {
                                rowOut[r] = at;
                                at += 1 + (nameOff[r + 1] - nameOff[r]) + 1 + body;
                        }
                } else if (format == KA_OUT_BLOCKS) {
                        const long long nb = ka_out_blocks(d.W), last = (long long)d.W - KA_OUT_BLOCK * (nb - 1);
                        at += (nb - 1) * ka_out_block_stride(d) + (long long)d.N * (d.nameMax + KA_OUT_NAME_PAD + last + 1) + 2;
                } else {
                        at += (long long)d.N * (ka_out_sto_row_len(d) + (hasRes ? ka_out_sto_gr_len(d) : 0)) + (hasCol ? ka_out_sto_gc_len(d) : 0) + 3;
                }
        }
        famOff[nFam] = at;
        if (format == KA_OUT_FASTA) rowOut.back() = at;
        return at;
}

} // namespace

struct ka_out_fam : KaStage {
        uint8_t gap = '-';
        int nFam = 0, numseq = 0;
        long long bytes = 0, cells = 0, cols = 0;      // of the packed rows; sum of N W; sum of W
        std::vector<KaOutFam> fams;                    // the families; a call fills its own fields in
        std::vector<int> rowFirst;                     // [nFam + 1]
        std::vector<uint8_t> names;                    // as given, or "seq0", "seq1", ... per family
        std::vector<long long> nameOff;                // [numseq + 1]
        // a call's tables: they are read by the uploads until the call's wait
        std::vector<long long> famOff, rowOut;
        std::vector<uint8_t> hdr;
        unsigned long long offender = KA_OUT_NONE;
        // the MSF row pass: once per handle
        bool haveRecs = false;
        std::vector<int> recs;                         // [numseq][2]: characters, prefix checksum
        DevBuf<KaOutFam> dFams;
        DevBuf<int> dRowFirst, dRecs;
        DevBuf<long long> dNameOff, dFamOff, dRowOut;
        DevBuf<uint8_t> dRows, dNames, dHdr, dOut;
        DevBuf<float> dRes, dCol;
        DevBuf<unsigned long long> dOffender;
        double st[KA_OUT_STATS] = {};                  // device ms of the row pass [0] and of the last fill [1]; [2], [3] the last writer's counters
        int rowLaunch = 0, rowSync = 0;                // of a row pass no writer has counted yet

        KaOutTab tab() const
        {
                KaOutTab a{};
                a.nFam = nFam; a.nRows = numseq; a.gap = gap;
                a.fams = dFams.p; a.famOff = dFamOff.p; a.rowOut = dRowOut.p; a.rowFirst = dRowFirst.p; a.rows = dRows.p;
                a.names = dNames.p; a.nameOff = dNameOff.p; a.hdr = dHdr.p; a.resConf = dRes.p; a.colConf = dCol.p;
                a.offender = dOffender.p; a.recs = dRecs.p; a.out = dOut.p;
                return a;
        }
        int create(const std::string& me, int n_fam, const int* fam_first, const uint8_t* rows, const int* alnlens, const uint8_t* names_in,
                   const long long* name_off);
        // out_layout over the handle's families as the call has filled them in: famOff, rowOut; the size
        long long layout(int format, int lineLength, bool hasRes, bool hasCol);
        int rowPass(const std::string& me);
        int msfHeaders(const std::string& me, const uint8_t* titles, const long long* title_off, const int* biotypes, const char* date);
        int write(const std::string& me, int format, int lineLength, const float* res, const float* col, uint8_t* out, long long cap,
                  long long* fam_off_out);
};

int ka_out_fam::create(const std::string& me, int n_fam, const int* fam_first, const uint8_t* rows, const int* alnlens, const uint8_t* names_in,
                       const long long* name_off)
{
        nFam = n_fam;
        numseq = fam_first[n_fam];
        rowFirst.assign(fam_first, fam_first + nFam + 1);
        out_families(n_fam, fam_first, alnlens, names_in, name_off, fams, names, nameOff, &bytes, &cells, &cols);
        if (open(2)) return KA_FAIL;
        if (dFams.alloc(nFam) || dRowFirst.alloc(rowFirst.size()) || dRows.alloc((size_t)bytes) || dNames.alloc(names.size()) ||
            dNameOff.alloc(nameOff.size()) || dFamOff.alloc((size_t)nFam + 1) || dRowOut.alloc((size_t)numseq + 1) || dOffender.alloc(1))
                return fail(me + ": out of device memory");
        HIPCHK(hipMemcpyAsync(dRowFirst.p, rowFirst.data(), sizeof(int) * rowFirst.size(), hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(dRows.p, rows, (size_t)bytes, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(dNames.p, names.data(), names.size(), hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(dNameOff.p, nameOff.data(), sizeof(long long) * nameOff.size(), hipMemcpyHostToDevice, stream));
        HIPCHK(hipStreamSynchronize(stream));                    // (the caller's rows are read no longer)
        return KA_OK;
}

long long ka_out_fam::layout(int format, int lineLength, bool hasRes, bool hasCol)
{
        return out_layout(fams, nameOff, format, lineLength, hasRes, hasCol, famOff, rowOut);
}

// The row pass over the whole batch, the records down, one wait.  They stay on the host.
int ka_out_fam::rowPass(const std::string& me)
{
        if (haveRecs) return KA_OK;
        HIPCHK(hipSetDevice(device));
        recs.assign((size_t)numseq * 2, 0);
        if (dRecs.alloc(recs.size())) return fail(me + ": out of device memory");
        HIPCHK(hipMemcpyAsync(dFams.p, fams.data(), sizeof(KaOutFam) * nFam, hipMemcpyHostToDevice, stream));
        HIPCHK(hipEventRecord(ev[0], stream));
        ka_out_run_rows(tab(), stream, &rowLaunch);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev[1], stream));
        HIPCHK(hipMemcpyAsync(recs.data(), dRecs.p, sizeof(int) * recs.size(), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        rowSync++;
        st[0] = ms();
        haveRecs = true;
        return KA_OK;
}

// write_msa_msf's header of every family, from the records, into hdr; the families' hdrOff / hdrLen
int ka_out_fam::msfHeaders(const std::string& me, const uint8_t* titles, const long long* title_off, const int* biotypes, const char* date)
{
        if (!titles || !title_off || !biotypes || !date) return fail(me + ": bad arguments");
        if (text_check(me, "the date", (const uint8_t*)date, (long long)std::strlen(date), 63)) return KA_FAIL;
        for (int f = 0; f < nFam; f++) {
                const std::string fam = me + ": family " + std::to_string(f);
                if (title_off[f + 1] < title_off[f]) return fail(me + ": title_off does not ascend");
                if (text_check(fam, "title", titles + title_off[f], title_off[f + 1] - title_off[f], KA_OUT_NAME_MAX)) return KA_FAIL;
                if (biotypes[f] != 0 && biotypes[f] != 1) return fail(fam + ": biotype " + std::to_string(biotypes[f]) + " is not 0 (protein) or 1 (DNA)");
        }
        if (rowPass(me)) return KA_FAIL;
        hdr.clear();
        std::vector<char> line;
        auto put = [&](const char* fmt, auto... args) {
                const int n = snprintf(nullptr, 0, fmt, args...);
                line.resize((size_t)n + 1);
                snprintf(line.data(), line.size(), fmt, args...);
                hdr.insert(hdr.end(), line.begin(), line.begin() + n);
                hdr.push_back('\n');
        };
        for (int f = 0; f < nFam; f++) {
                KaOutFam& d = fams[f];
                const int* r = &recs[(size_t)d.firstRow * 2];
                const std::string title(titles + title_off[f], titles + title_off[f + 1]);
                int check = 0;
                for (int i = 0; i < d.N; i++) check = (check + r[2 * i + 1]) % 10000;
                d.hdrOff = (long long)hdr.size();
                put("%s", kMsfBanner[biotypes[f]]);
                put("%s", "");
                put(" %s  MSF: %d  Type: %c  %s  Check: %d  ..", title.c_str(), r[0], kMsfType[biotypes[f]], date, check);
                put("%s", "");
                for (int i = 0; i < d.N; i++) {
                        const int row = d.firstRow + i;
                        const std::string name(names.begin() + nameOff[row], names.begin() + nameOff[row + 1]);
                        put(" Name: %-*.*s  Len:  %5d  Check: %4d  Weight: %.2f", d.nameMax, d.nameMax, name.c_str(), r[0], r[2 * i + 1], 1.0);
                }
                put("%s", "");
                put("%s", "//");
                put("%s", "");
                if ((long long)hdr.size() - d.hdrOff > INT32_MAX) return fail(me + ": family " + std::to_string(f) + ": the header holds 2^31 bytes or more");
                d.hdrLen = (int)((long long)hdr.size() - d.hdrOff);
        }
        return KA_OK;
}

// The call's tables up, one launch, text and offender record down, one wait.  The families' header fields and `hdr` are
// the caller's (of this unit) to set before.
int ka_out_fam::write(const std::string& me, int format, int lineLength, const float* res, const float* col, uint8_t* out, long long cap,
                      long long* fam_off_out)
{
        const long long total = layout(format, lineLength, res != nullptr, col != nullptr);
        if (cap < total) return fail(me + ": " + std::to_string(cap) + " bytes do not hold the text (" + std::to_string(total) + ")");
        if (!out) return fail(me + ": bad arguments");
        if (total > (1ll << 39)) return fail(me + ": a text of " + std::to_string(total) + " bytes; a call writes 2^39 at most");
        HIPCHK(hipSetDevice(device));
        if (dOut.alloc((size_t)((total + 3) / 4 * 4)) || dHdr.alloc(std::max<size_t>(hdr.size(), 1)) || (res && dRes.alloc((size_t)cells)) ||
            (col && dCol.alloc((size_t)cols)))
                return fail(me + ": out of device memory");
        nLaunch = rowLaunch; nSync = rowSync;                    // (a row pass that ran for this call counts with it)
        rowLaunch = rowSync = 0;
        offender = KA_OUT_NONE;
        HIPCHK(hipMemcpyAsync(dFams.p, fams.data(), sizeof(KaOutFam) * nFam, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(dFamOff.p, famOff.data(), sizeof(long long) * famOff.size(), hipMemcpyHostToDevice, stream));
        if (format == KA_OUT_FASTA) HIPCHK(hipMemcpyAsync(dRowOut.p, rowOut.data(), sizeof(long long) * rowOut.size(), hipMemcpyHostToDevice, stream));
        if (!hdr.empty()) HIPCHK(hipMemcpyAsync(dHdr.p, hdr.data(), hdr.size(), hipMemcpyHostToDevice, stream));
        if (res) HIPCHK(hipMemcpyAsync(dRes.p, res, sizeof(float) * (size_t)cells, hipMemcpyHostToDevice, stream));
        if (col) HIPCHK(hipMemcpyAsync(dCol.p, col, sizeof(float) * (size_t)cols, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(dOffender.p, &offender, sizeof offender, hipMemcpyHostToDevice, stream));
        KaOutTab a = tab();
        a.format = format; a.lineLength = lineLength; a.hasRes = res != nullptr; a.hasCol = col != nullptr; a.total = total;
        HIPCHK(hipEventRecord(ev[0], stream));
        ka_out_run_fill(a, stream, &nLaunch);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev[1], stream));
        HIPCHK(hipMemcpyAsync(out, dOut.p, (size_t)total, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipMemcpyAsync(&offender, dOffender.p, sizeof offender, hipMemcpyDeviceToHost, stream));
        if (wait()) return KA_FAIL;
        st[1] = ms();
        if (offender != KA_OUT_NONE) {
                std::memset(out, 0, (size_t)total);              // no text is handed out
                int f = nFam - 1;
                while (f > 0 && (unsigned long long)fams[f].keyBase > offender) f--;
                const KaOutFam& d = fams[f];
                const long long k = (long long)offender - d.keyBase, seq = k / d.W, c = k % d.W;
                const float v = seq < d.N ? res[d.confOff + k] : col[d.colOff + c];
                char num[32];
                snprintf(num, sizeof num, "%.9g", (double)v);
                const std::string at = me + ": family " + std::to_string(f) + (seq < d.N ? ", sequence " + std::to_string(seq) : std::string()) + ", column " + std::to_string(c);
                return fail(at + ": " + (seq < d.N ? "confidence " : "column confidence ") + num + " outside [0, 1]");
        }
        if (fam_off_out) std::copy(famOff.begin(), famOff.end(), fam_off_out);
        return KA_OK;
}

extern "C" int ka_out_pp_char(float confidence)
{
        return ka_out_pp(confidence);
}

extern "C" int ka_out_fam_check(int n_fam, const int* fam_first, const uint8_t* rows, const int* alnlens, const uint8_t* names, const long long* name_off)
{
        return out_check("ka_out_fam_check", n_fam, fam_first, rows, alnlens, names, name_off);
}

extern "C" int ka_out_fam_text_sizes(int n_fam, const int* fam_first, const int* alnlens, const long long* name_off, int format, int param,
                                     long long* fam_off_out)
{
        const std::string me("ka_out_fam_text_sizes");
        if (!fam_off_out) return fail(me + ": bad arguments");
        const uint8_t none = 0;
        if (ka_sum_check_named(me, n_fam, fam_first, &none, alnlens)) return KA_FAIL;    // (the rows themselves are not read)
        if (name_off)
                for (int i = 0; i < fam_first[n_fam]; i++)
                        if (name_off[i + 1] - name_off[i] < 1 || name_off[i + 1] - name_off[i] > KA_OUT_NAME_MAX)
                                return fail(me + ": a name holds 1 to 255 bytes");
        if (format < 0 || format > 2) return fail(me + ": format " + std::to_string(format) + " is not 0 (FASTA), 1 (Clustal) or 2 (Stockholm)");
        if (format == 0 && param < 1) return fail(me + ": line_length " + std::to_string(param) + "; a line holds one column at least");
        if (format == 1 && (param < 0 || param > KA_OUT_NAME_MAX)) return fail(me + ": header of " + std::to_string(param) + " bytes; it holds 255 at most");
        if (format == 2 && (param < 1 || param > 3)) return fail(me + ": confidences " + std::to_string(param) + " are not 1 (residue), 2 (column) or 3 (both)");
        std::vector<KaOutFam> fams;
        std::vector<uint8_t> names;
        std::vector<long long> nameOff, famOff, rowOut;
        long long bytes, cells, cols;
        out_families(n_fam, fam_first, alnlens, nullptr, name_off, fams, names, nameOff, &bytes, &cells, &cols);
        for (auto& d : fams) d.hdrLen = format == 0 ? 0 : format == 1 ? param + 2 : (int)sizeof kStockholm - 1;
        out_layout(fams, nameOff, format == 0 ? KA_OUT_FASTA : format == 1 ? KA_OUT_BLOCKS : KA_OUT_STOCKHOLM, param, format == 2 && (param & 1),
                   format == 2 && (param & 2), famOff, rowOut);
        std::copy(famOff.begin(), famOff.end(), fam_off_out);
        return KA_OK;
}

extern "C" int ka_out_fam_create(ka_ctx* ctx, int n_fam, const int* fam_first, const uint8_t* rows, const int* alnlens, int gap_char,
                                 const uint8_t* names, const long long* name_off, ka_out_fam** out)
{
        const std::string me("ka_out_fam_create");
        if (!ctx || !out || gap_char < 0 || gap_char > 255) return fail(me + ": bad arguments");
        *out = nullptr;
        if (out_check(me, n_fam, fam_first, rows, alnlens, names, name_off)) return KA_FAIL;
        std::unique_ptr<ka_out_fam> h(new ka_out_fam);
        if (h->attach(ctx)) return fail(me + ": bad context");
        h->gap = (uint8_t)gap_char;
        if (h->create(me, n_fam, fam_first, rows, alnlens, names, name_off)) return h->refused();
        *out = h.release();
        return KA_OK;
}

extern "C" void ka_out_fam_destroy(ka_out_fam* h)
{
        ka_stage_destroy(h);
}

// ---- FASTA ----
static int fasta_begin(const std::string& me, ka_out_fam* h, int line_length)
{
        if (!h) return fail(me + ": bad arguments");
        if (line_length < 1) return fail(me + ": line_length " + std::to_string(line_length) + "; a line holds one column at least");
        for (auto& d : h->fams) d.hdrOff = d.hdrLen = 0;
        h->hdr.clear();
        return KA_OK;
}

extern "C" long long ka_out_fam_fasta_size(ka_out_fam* h, int line_length)
{
        if (fasta_begin("ka_out_fam_fasta_size", h, line_length)) return -1;
        return h->layout(KA_OUT_FASTA, line_length, false, false);
}

extern "C" int ka_out_fam_fasta(ka_out_fam* h, int line_length, uint8_t* out, long long cap, long long* fam_off_out)
{
        const std::string me("ka_out_fam_fasta");
        if (fasta_begin(me, h, line_length)) return KA_FAIL;
        return h->write(me, KA_OUT_FASTA, line_length, nullptr, nullptr, out, cap, fam_off_out);
}

// ---- Clustal ----
static int clustal_begin(const std::string& me, ka_out_fam* h, const char* header)
{
        if (!h || !header) return fail(me + ": bad arguments");
        const size_t n = std::strlen(header);
        if (n > (size_t)KA_OUT_NAME_MAX) return fail(me + ": header of " + std::to_string(n) + " bytes; it holds 255 at most");
        h->hdr.assign(header, header + n);
        h->hdr.push_back('\n');                                  // the header line, then the empty line
        h->hdr.push_back('\n');
        for (auto& d : h->fams) { d.hdrOff = 0; d.hdrLen = (int)n + 2; }
        return KA_OK;
}

extern "C" long long ka_out_fam_clustal_size(ka_out_fam* h, const char* header)
{
        if (clustal_begin("ka_out_fam_clustal_size", h, header)) return -1;
        return h->layout(KA_OUT_BLOCKS, 0, false, false);
}

extern "C" int ka_out_fam_clustal(ka_out_fam* h, const char* header, uint8_t* out, long long cap, long long* fam_off_out)
{
        const std::string me("ka_out_fam_clustal");
        if (clustal_begin(me, h, header)) return KA_FAIL;
        return h->write(me, KA_OUT_BLOCKS, 0, nullptr, nullptr, out, cap, fam_off_out);
}

// ---- MSF ----
extern "C" int ka_out_fam_msf_records(ka_out_fam* h, int* recs_out, int* fam_check_out)
{
        if (!h) return fail("ka_out_fam_msf_records: bad arguments");
        if (h->rowPass("ka_out_fam_msf_records")) return KA_FAIL;
        if (recs_out) std::copy(h->recs.begin(), h->recs.end(), recs_out);
        if (fam_check_out)
                for (int f = 0; f < h->nFam; f++) {
                        int check = 0;
                        for (int r = h->rowFirst[f]; r < h->rowFirst[f + 1]; r++) check = (check + h->recs[(size_t)r * 2 + 1]) % 10000;
                        fam_check_out[f] = check;
                }
        return KA_OK;
}

extern "C" long long ka_out_fam_msf_size(ka_out_fam* h, const uint8_t* titles, const long long* title_off, const int* biotypes, const char* date)
{
        if (!h) return fail("ka_out_fam_msf_size: bad arguments"), -1;
        if (h->msfHeaders("ka_out_fam_msf_size", titles, title_off, biotypes, date)) return -1;
        return h->layout(KA_OUT_BLOCKS, 0, false, false);
}

extern "C" int ka_out_fam_msf(ka_out_fam* h, const uint8_t* titles, const long long* title_off, const int* biotypes, const char* date, uint8_t* out,
                              long long cap, long long* fam_off_out)
{
        const std::string me("ka_out_fam_msf");
        if (!h) return fail(me + ": bad arguments");
        if (h->msfHeaders(me, titles, title_off, biotypes, date)) return KA_FAIL;
        return h->write(me, KA_OUT_BLOCKS, 0, nullptr, nullptr, out, cap, fam_off_out);
}

// ---- Stockholm ----
static int stockholm_begin(const std::string& me, ka_out_fam* h, bool has_res, bool has_col)
{
        if (!h) return fail(me + ": bad arguments");
        if (!has_res && !has_col)
                return fail(me + ": without confidences the reference writes Stockholm through Biopython, which this stage does not restate: "
                                 "give residue_conf, column_conf or both");
        h->hdr.assign(kStockholm, kStockholm + sizeof kStockholm - 1);
        for (auto& d : h->fams) { d.hdrOff = 0; d.hdrLen = (int)sizeof kStockholm - 1; }
        return KA_OK;
}

extern "C" long long ka_out_fam_stockholm_size(ka_out_fam* h, int has_residue_conf, int has_column_conf)
{
        if (stockholm_begin("ka_out_fam_stockholm_size", h, has_residue_conf != 0, has_column_conf != 0)) return -1;
        return h->layout(KA_OUT_STOCKHOLM, 0, has_residue_conf != 0, has_column_conf != 0);
}

extern "C" int ka_out_fam_stockholm(ka_out_fam* h, const float* residue_conf, const float* column_conf, uint8_t* out, long long cap,
                                    long long* fam_off_out)
{
        const std::string me("ka_out_fam_stockholm");
        if (stockholm_begin(me, h, residue_conf != nullptr, column_conf != nullptr)) return KA_FAIL;
        return h->write(me, KA_OUT_STOCKHOLM, 0, residue_conf, column_conf, out, cap, fam_off_out);
}

extern "C" int ka_out_fam_stats(ka_out_fam* h, double* out4)
{
        if (!h) return fail("ka_out_fam_stats: bad arguments");
        h->st[2] = h->nLaunch; h->st[3] = h->nSync;
        if (out4) std::copy_n(h->st, KA_OUT_STATS, out4);
        return KA_OK;
}
