// ka_cmp_fam.cpp -- scoring a batch of families, each against its own reference alignment: the ka_cmp_fam handle of the
// C ABI, a front over the comparison stage's core (ka_cmp_core.h, ka_cmp.cpp) with one reference and one job per family
// and the rows packed as ka_batch_rows hands them out (a row of W columns W + 1 bytes), uploaded in one copy.
//
// Every check runs on the host before anything is launched (cmp_fam_check; ka_cmp_fam_check is its public form), with
// the functions the one-family calls use (KaSeqSet::set, ka_msa_check_rows): a family is refused with the cause it is
// refused with alone.
#include "ka_cmp_core.h"

namespace {

// a packed batch on the host alone: the families, their sequences and their rows
int cmp_fam_check(const char* who, int n_fam, const int* fam_first, const int* lens, const uint8_t* rows, const int* alnlens)
{
        const std::string me(who);
        if (!lens || !rows || !alnlens) return fail(me + ": bad arguments");
        if (ka_fam_check_first(me, n_fam, fam_first)) return KA_FAIL;
        const std::string why = "the position maps hold at most " + std::to_string(KA_CMP_MAX_RES);
        long long residues = 0, cols = 0, off = 0;
        for (int f = 0; f < n_fam; f++) {
                const std::string fam = me + ": family " + std::to_string(f);
                const int N = fam_first[f + 1] - fam_first[f];
                if (N < 2) return fail(fam + ": " + std::to_string(N) + " sequences; a comparison needs two at least");
                KaSeqSet q;                                      // (host side only: nothing to release)
                if (q.set(fam.c_str(), N, lens + fam_first[f], KA_CMP_MAX_RES, why.c_str())) return KA_FAIL;
                if (ka_msa_check_rows(fam.c_str(), q, rows + off, (long long)alnlens[f] + 1, alnlens[f])) return KA_FAIL;
                residues += q.T;
                cols += alnlens[f];
                off += (long long)N * (alnlens[f] + 1);
                if (residues > INT32_MAX) return fail(me + ": more than 2^31 - 1 residues in the batch");
                if (cols > INT32_MAX) return fail(me + ": more than 2^31 - 1 columns in the batch");
        }
        return KA_OK;
}

// the packed rows of `alnlens` in one copy
KaCmpUpload packed(const uint8_t* rows, const int* fam_first, int n_fam, const int* alnlens)
{
        const long long bytes = ka_fam_row_bytes(n_fam, fam_first, alnlens);
        return [=](uint8_t* dst, hipStream_t s) {
                HIPCHK(hipMemcpyAsync(dst, rows, (size_t)bytes, hipMemcpyHostToDevice, s));
                return (int)KA_OK;
        };
}

} // namespace

struct ka_cmp_fam {
        KaCmpCore core;
        std::vector<int> famFirst;
};

extern "C" int ka_cmp_fam_check(int n_fam, const int* fam_first, const int* lens, const uint8_t* rows, const int* alnlens)
{
        return cmp_fam_check("ka_cmp_fam_check", n_fam, fam_first, lens, rows, alnlens);
}

extern "C" int ka_cmp_fam_create(ka_ctx* ctx, int n_fam, const int* fam_first, const int* lens, const uint8_t* ref_rows, const int* ref_alnlens,
                                 ka_cmp_fam** out)
{
        if (!ctx || !out) return fail("ka_cmp_fam_create: bad arguments");
        *out = nullptr;
        if (cmp_fam_check("ka_cmp_fam_create", n_fam, fam_first, lens, ref_rows, ref_alnlens)) return KA_FAIL;
        std::unique_ptr<ka_cmp_fam> h(new ka_cmp_fam);
        if (h->core.attach(ctx)) return fail("ka_cmp_fam_create: bad context");
        h->famFirst.assign(fam_first, fam_first + n_fam + 1);
        if (h->core.create("ka_cmp_fam_create", "family", n_fam, fam_first, lens, ref_alnlens, 1, packed(ref_rows, fam_first, n_fam, ref_alnlens)))
                return KA_FAIL;
        *out = h.release();
        return KA_OK;
}

extern "C" void ka_cmp_fam_destroy(ka_cmp_fam* h)
{
        if (!h) return;
        h->core.close();
        delete h;
}

extern "C" int ka_cmp_fam_set_masks(ka_cmp_fam* h, const float* max_gap_frac, const int* masks, const long long* mask_off)
{
        if (!h) return fail("ka_cmp_fam_set_masks: bad arguments");
        const int F = (int)h->core.refs.size();
        std::vector<float> frac(F, -1.0f);
        std::vector<long long> off(F, -1);
        if (max_gap_frac) std::copy_n(max_gap_frac, F, frac.begin());
        long long n = 0;                                         // ints of `masks` in use
        if (masks && mask_off)
                for (int f = 0; f < F; f++) {
                        if (mask_off[f] < 0) continue;
                        off[f] = mask_off[f];
                        n = std::max(n, mask_off[f] + h->core.refs[f].r.W);
                }
        return h->core.set_rule("ka_cmp_fam_set_masks", frac.data(), masks, off.data(), n);
}

extern "C" int ka_cmp_fam_score(ka_cmp_fam* h, const uint8_t* test_rows, const int* test_alnlens, long long* counts_out, double* scores_out,
                                float* sp_out)
{
        if (!h) return fail("ka_cmp_fam_score: bad arguments");
        const int F = (int)h->core.refs.size();
        if (cmp_fam_check("ka_cmp_fam_score", F, h->famFirst.data(), h->core.lens.data(), test_rows, test_alnlens)) return KA_FAIL;
        std::fill_n(h->core.st + 1, KA_CMP_STATS - 1, 0.0);
        return h->core.score("ka_cmp_fam_score", "family", F, nullptr, test_alnlens, 1, packed(test_rows, h->famFirst.data(), F, test_alnlens),
                             counts_out, scores_out, sp_out);
}

extern "C" int ka_cmp_fam_stats(ka_cmp_fam* h, double* stats_out)
{
        if (!h) return fail("ka_cmp_fam_stats: bad arguments");
        if (stats_out) std::copy_n(h->core.st, KA_CMP_STATS, stats_out);
        return KA_OK;
}

extern "C" int ka_cmp_fam_detail(ka_cmp_fam* h, const uint8_t* test_rows, const int* test_alnlens, int* res_counts, int* tcol_residues,
                                 long long* tcol_common, uint8_t* tcol_correct, int* rcol_residues, long long* rcol_common, uint8_t* rcol_correct)
{
        if (!h) return fail("ka_cmp_fam_detail: bad arguments");
        std::fill_n(h->core.dst, KA_CMP_DETAIL_STATS, 0.0);
        const int F = (int)h->core.refs.size();
        if (cmp_fam_check("ka_cmp_fam_detail", F, h->famFirst.data(), h->core.lens.data(), test_rows, test_alnlens)) return KA_FAIL;
        return h->core.detail("ka_cmp_fam_detail", "family", test_alnlens, 1, packed(test_rows, h->famFirst.data(), F, test_alnlens), res_counts,
                              tcol_residues, tcol_common, tcol_correct, rcol_residues, rcol_common, rcol_correct);
}

extern "C" int ka_cmp_fam_detail_stats(ka_cmp_fam* h, double* out5)
{
        if (!h) return fail("ka_cmp_fam_detail_stats: bad arguments");
        if (out5) std::copy_n(h->core.dst, KA_CMP_DETAIL_STATS, out5);
        return KA_OK;
}
