"""The family table's rule -- fam_first ascends from 0 to numseq, no family is empty -- reads the same at every public entry
that takes a table and needs no context: "<entry name>: " and one of two texts.  No GPU: every call is refused on the host."""
import ctypes as C

import numpy as np
import pytest

ASCEND, EMPTY = "fam_first does not ascend from 0 to numseq", "empty family"
BAD = (([1, 3, 5], ASCEND), ([0, 4, 3], ASCEND), ([0, 3, 3], EMPTY))       # first != 0, descending, an empty family
ints, longs, octets = np.zeros(8, np.int32), np.zeros(8, np.int64), np.zeros(64, np.uint8)


def entries():
    from kalign_amd import api
    p = api._ptr
    dist = api.DIST_FN(lambda user, n, ia, ib, out: 1)
    return {
        "ka_sum_fam_check": lambda L, ff: L.ka_sum_fam_check(2, ff, p(octets), p(ints)),
        "ka_sum_fam_identity_entries": lambda L, ff: L.ka_sum_fam_identity_entries(2, ff),
        "ka_ens_fam_check": lambda L, ff: L.ka_ens_fam_check(2, ff, p(ints), p(octets), p(ints)),
        "ka_cmp_fam_check": lambda L, ff: L.ka_cmp_fam_check(2, ff, p(ints), p(octets), p(ints)),
        "ka_in_fam_check": lambda L, ff: L.ka_in_fam_check(2, ff, p(longs), 0),
        "ka_in_order": lambda L, ff: L.ka_in_order(2, ff, p(ints), None, None, p(ints)),
        "ka_cod_fam_check": lambda L, ff: L.ka_cod_fam_check(2, ff, p(longs), 0),
        "ka_out_fam_check": lambda L, ff: L.ka_out_fam_check(2, ff, p(octets), p(ints), None, None),
        "ka_guide_forest_from": lambda L, ff: L.ka_guide_forest_from(2, ff, p(ints), dist, None, 1, None, p(ints), None, None),
    }


NAMES = ("ka_sum_fam_check", "ka_sum_fam_identity_entries", "ka_ens_fam_check", "ka_cmp_fam_check", "ka_in_fam_check", "ka_in_order",
         "ka_cod_fam_check", "ka_out_fam_check", "ka_guide_forest_from")


@pytest.mark.parametrize("name", NAMES)
def test_a_bad_table_reads_the_same_everywhere(name):
    import kalign_amd
    from kalign_amd import api
    L = kalign_amd.load_library()
    call = entries()[name]
    for first, text in BAD:
        ff = np.array(first, np.int32)
        rc = call(L, api._ptr(ff))
        assert rc == (-1 if name == "ka_sum_fam_identity_entries" else 1), (name, first)
        assert L.ka_last_error().decode() == name + ": " + text, (name, first)
