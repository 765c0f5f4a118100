// fam_host_check.cpp -- a stand-alone program for sanitizer builds of what the stages of a batch of families share on the host
// (kalign_amd/csrc/ka_fam.h) and of the host-only builds of the input and codon stages that call it: the family table's rule at
// its edges, the words that name a sequence, the size of a packed batch, the lent check, the order.  Prints "ok".  Needs no
// GPU and no HIP header.  Build it from kalign_amd/csrc:
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -DKA_IN_HOST_ONLY -DKA_COD_HOST_ONLY \
//         -I../../include -I. ../../tools/fam_host_check.cpp ka_in.cpp ka_cod.cpp -o fam_host_check
#include <cstdio>
#include <string>
#include <vector>
#include "ka_fam.h"

// what the units take from the rest of the library: the error text
static std::string g_err;
int fail(const std::string& m) { g_err = m; return KA_FAIL; }

static int bad(const char* what)
{
        std::printf("%s: %s\n", what, g_err.c_str());
        return 1;
}

int main()
{
        const std::string me = "fam_host_check";
        // the rule, at arrays that hold exactly n_fam + 1 ints: a read past one is the sanitizer's to report
        const std::vector<int> good{ 0, 2, 3, 7 }, shifted{ 1, 2, 3, 7 }, down{ 0, 2, 1, 7 }, empty{ 0, 2, 2, 7 }, one{ 0, 1 };
        if (ka_fam_check_first(me, 3, good.data()) || ka_fam_check_first(me, 1, one.data())) return bad("a good table was refused");
        if (!ka_fam_check_first(me, 0, good.data()) || g_err != me + ": bad arguments") return bad("n_fam 0");
        if (!ka_fam_check_first(me, 3, nullptr) || g_err != me + ": bad arguments") return bad("no table");
        if (!ka_fam_check_first(me, 3, shifted.data()) || g_err != me + ": fam_first does not ascend from 0 to numseq") return bad("first != 0");
        if (!ka_fam_check_first(me, 3, down.data()) || g_err != me + ": fam_first does not ascend from 0 to numseq") return bad("descending");
        if (!ka_fam_check_first(me, 3, empty.data()) || g_err != me + ": empty family") return bad("empty family");
        if (ka_fam_where(me, 2, 5) != "fam_host_check: family 2, sequence 5") return bad("where");
        const std::vector<int> widths{ 4, 0, 2147483647 };
        if (ka_fam_row_bytes(3, good.data(), widths.data()) != 2 * 5 + 1 * 1 + 4 * 2147483648ll) return bad("row bytes");

        // the lent check and the entries over it, in the host-only builds of the two stages
        const std::vector<long long> off{ 0, 4, 4, 9, 9, 9, 12, 20 };
        if (ka_in_fam_check(3, good.data(), off.data(), 20) || ka_cod_fam_check(3, good.data(), off.data(), 20)) return bad("a good batch was refused");
        if (!ka_cod_fam_check(3, empty.data(), off.data(), 20) || g_err != "ka_cod_fam_check: empty family") return bad("the lent check's name");
        if (!ka_in_fam_check(3, good.data(), off.data(), 19) || g_err != "ka_in_fam_check: seq_off does not ascend from 0 to n_bytes") return bad("seq_off");
        const std::vector<int> residues{ 3, 9, 5, 1, 1, 8, 8 };
        std::vector<int> order(7, -1);
        if (ka_in_order(3, good.data(), residues.data(), nullptr, nullptr, order.data())) return bad("order");
        if (order != std::vector<int>{ 1, 0, 2, 5, 6, 3, 4 }) return bad("order: the result");
        if (!ka_in_order(3, down.data(), residues.data(), nullptr, nullptr, order.data()) || g_err != "ka_in_order: fam_first does not ascend from 0 to numseq")
                return bad("order: a bad table");
        std::printf("ok\n");
        return 0;
}
