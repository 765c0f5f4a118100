// ka_poar.cpp -- the reader's side of the ensemble's POAR file (poar_table_read, lib/src/poar.c:254-325), host only: no
// context, no GPU.  The reference trusts the file (a count or key that does not fit the input indexes out of bounds in
// build_consensus); here every word is checked against the caller's sequences before anything is built from it.
//
//     "POAR" | version 1 | numseq | n_alignments | per pair i < j: n_entries | n_entries x { ri << 20 | rj ; member mask }
#include "ka_ctx.h"
#include "ka_ens.h"

namespace {

uint32_t word(const uint8_t* p)          // little endian, any alignment
{
        return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

std::string hex(uint32_t v)
{
        char b[16];
        std::snprintf(b, sizeof b, "0x%08X", v);
        return b;
}

} // namespace

int ka_poar_parse(const uint8_t* image, long long nBytes, int numseq, const int* lens, int* nRuns, long long* entries, std::vector<long long>* pairStart)
{
        const std::string who = "POAR table: ";
        if (!image || !lens || numseq < 1 || nBytes < 0) return fail(who + "bad arguments");
        for (int s = 0; s < numseq; s++)
                if (lens[s] < 0 || lens[s] > KA_ENS_MAX_RES)
                        return fail(who + "sequence " + std::to_string(s) + " has " + std::to_string(lens[s]) + " residues; a key holds residue indices below " + std::to_string(KA_ENS_MAX_RES));
        if (nBytes < 16) return fail(who + std::to_string(nBytes) + " bytes, shorter than the 16-byte header (truncated)");
        if (word(image) != 0x524F4150u) return fail(who + "wrong magic " + hex(word(image)) + " (a POAR file starts with 0x524F4150, \"POAR\")");
        if (word(image + 4) != 1u) return fail(who + "version " + std::to_string(word(image + 4)) + " not supported (only version 1)");
        if (word(image + 8) != (uint32_t)numseq)
                return fail(who + "numseq " + std::to_string(word(image + 8)) + " in the file, " + std::to_string(numseq) + " sequences given");
        const uint32_t R = word(image + 12);
        if (R < 1 || R > KA_ENS_MAX_RUNS) return fail(who + "n_alignments " + std::to_string(R) + " outside 1.." + std::to_string(KA_ENS_MAX_RUNS));
        const uint32_t over = R == 32 ? 0u : ~0u << R;          // the bits no member owns
        if (pairStart) { pairStart->clear(); pairStart->reserve((size_t)numseq * (numseq - 1) / 2 + 1); }
        long long at = 16, total = 0;
        for (int i = 0; i + 1 < numseq; i++)
                for (int j = i + 1; j < numseq; j++) {
                        auto pairName = [&] { return "pair (" + std::to_string(i) + ", " + std::to_string(j) + ")"; };    // (errors only)
                        if (at + 4 > nBytes) return fail(who + "truncated: the file ends before the entry count of " + pairName());
                        const long long n = word(image + at);
                        at += 4;
                        if (n > (nBytes - at) / 8) return fail(who + "truncated: " + pairName() + " counts " + std::to_string(n) + " entries, " + std::to_string(nBytes - at) + " bytes are left");
                        if (pairStart) pairStart->push_back(total);
                        uint32_t prev = 0;
                        for (long long x = 0; x < n; x++, at += 8) {
                                const uint32_t key = word(image + at), mask = word(image + at + 4);
                                auto where = [&] { return pairName() + " entry " + std::to_string(x); };
                                if ((int)(key >> 20) >= lens[i])
                                        return fail(who + where() + ": residue ri = " + std::to_string(key >> 20) + " but sequence " + std::to_string(i) + " has " + std::to_string(lens[i]));
                                if ((int)(key & 0xFFFFFu) >= lens[j])
                                        return fail(who + where() + ": residue rj = " + std::to_string(key & 0xFFFFFu) + " but sequence " + std::to_string(j) + " has " + std::to_string(lens[j]));
                                if (x > 0 && key <= prev) return fail(who + where() + ": keys not strictly ascending (" + hex(key) + " after " + hex(prev) + ")");
                                if (mask == 0) return fail(who + where() + ": mask 0 (an entry is held by at least one member)");
                                if (mask & over) return fail(who + where() + ": mask " + hex(mask) + " has a bit at or above n_alignments = " + std::to_string(R));
                                prev = key;
                        }
                        total += n;
                }
        if (at != nBytes) return fail(who + std::to_string(nBytes - at) + " bytes after the last pair (longer than its counts imply)");
        if (pairStart) pairStart->push_back(total);
        if (nRuns) *nRuns = (int)R;
        if (entries) *entries = total;
        return KA_OK;
}

extern "C" int ka_poar_check_image(const uint8_t* image, long long n_bytes, int numseq, const int* lens, int* n_runs_out, long long* entries_out)
{
        return ka_poar_parse(image, n_bytes, numseq, lens, n_runs_out, entries_out, nullptr);
}
