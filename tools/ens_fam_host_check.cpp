// ens_fam_host_check.cpp -- a stand-alone program for sanitizer builds of the host-only parts of ka_ens_fam.cpp (the check of
// a packed batch and the seam ka_debug_ens_fam_consensus_host): it feeds them a random batch of 40 small families with 16
// threads, compares with one thread, and prints "ok".  Needs no GPU.  Build it from kalign_amd/csrc with the host side
// instrumented, once per sanitizer set (address,undefined -- then thread):
//     hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -I../../include -I. \
//           -x hip ../../tools/ens_fam_host_check.cpp ka_ens_fam.cpp ka_ens.cpp ka_ens.hip ka_poar.cpp ka_poar.hip ka_msa.hip -o ens_fam_host_check
// (ka_ens.cpp holds the host core ka_ens_fam.cpp is a front of, and with it the one-family front and its table passes)
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "ka_ctx.h"                        // fail(), ka_ctx
#include "kalign_amd.h"

// what the two units take from the rest of the library: the error text, and the context (never reached here)
static std::string g_err;
int fail(const std::string& m) { g_err = m; return KA_FAIL; }
int ka_ctx_device_stream(ka_ctx*, int*, hipStream_t*) { return 1; }

int main()
{
        std::mt19937 rng(40);
        auto pick = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
        const int F = 40;
        std::vector<int> first{ 0 }, lens, widths;
        std::vector<long long> candFirst{ 0 };
        std::vector<int> cand;
        std::vector<uint8_t> letters, rows;
        for (int f = 0; f < F; f++) {
                const int N = pick(2, 12), W = 48;
                std::vector<int> o(N + 1, 0);
                std::vector<std::vector<int>> cols(N);
                for (int s = 0; s < N; s++) {
                        const int L = pick(5, 40);
                        lens.push_back(L);
                        o[s + 1] = o[s] + L;
                        // a random placement of the residues in W columns: one alignment of the family
                        std::vector<int> all(W);
                        for (int c = 0; c < W; c++) all[c] = c;
                        for (int c = 0; c < L; c++) std::swap(all[c], all[c + (int)(rng() % (unsigned)(W - c))]);
                        cols[s].assign(all.begin(), all.begin() + L);
                        std::sort(cols[s].begin(), cols[s].end());
                        std::vector<uint8_t> row(W + 1, '-');
                        row[W] = 0;
                        for (int r = 0; r < L; r++) { row[cols[s][r]] = (uint8_t)('A' + pick(0, 19)); letters.push_back(row[cols[s][r]]); }
                        rows.insert(rows.end(), row.begin(), row.end());
                }
                // candidates: the aligned pairs of that alignment, and as many random pairs (most of them refused by the greedy)
                for (int i = 0; i < N; i++)
                        for (int j = i + 1; j < N; j++)
                                for (int ri = 0; ri < (int)cols[i].size(); ri++)
                                        for (int rj = 0; rj < (int)cols[j].size(); rj++)
                                                if (cols[i][ri] == cols[j][rj] || rng() % 97 == 0) { cand.push_back(o[i] + ri); cand.push_back(o[j] + rj); }
                candFirst.push_back((long long)cand.size() / 2);
                first.push_back(first.back() + N);
                widths.push_back(W);
        }
        if (ka_ens_fam_check(F, first.data(), lens.data(), rows.data(), widths.data())) { std::printf("check: %s\n", g_err.c_str()); return 1; }
        lens[3]++;
        if (!ka_ens_fam_check(F, first.data(), lens.data(), rows.data(), widths.data()) || g_err.find("family 0: row 3") == std::string::npos) {
                std::printf("a wrong letter count was not refused: %s\n", g_err.c_str());
                return 1;
        }
        lens[3]--;
        long long cap = 0;
        for (int f = 0; f < F; f++) {
                int T = 0;
                for (int s = first[f]; s < first[f + 1]; s++) T += lens[s];
                cap += (long long)(first[f + 1] - first[f]) * (T + 1);
        }
        std::vector<uint8_t> out1((size_t)cap, 1), out16((size_t)cap, 1);
        std::vector<int> w1(F), w16(F);
        if (ka_debug_ens_fam_consensus_host(F, first.data(), lens.data(), candFirst.data(), cand.data(), letters.data(), 1, w1.data(), out1.data(), cap) ||
            ka_debug_ens_fam_consensus_host(F, first.data(), lens.data(), candFirst.data(), cand.data(), letters.data(), 16, w16.data(), out16.data(), cap)) {
                std::printf("seam: %s\n", g_err.c_str());
                return 1;
        }
        if (w1 != w16 || out1 != out16) { std::printf("1 and 16 threads differ\n"); return 1; }
        std::printf("ok: %d families, %lld candidates\n", F, candFirst.back());
        return 0;
}
