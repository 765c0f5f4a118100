"""The host side of the identity pass of the summary stage: the names and the ABI revision, ka_sum_fam_identity_entries on
valid and refused family tables (messages compared as strings), and the numpy restatement (tests/sum_identity_restate.py)
against every golden recorded from python-kalign's kalign.utils.pairwise_identity_matrix (tests/golden/idm_*.npz: floats
with ==) and against the family sums of the summary restatement (tests/sum_restate.py).  No GPU."""
import glob
import os

import numpy as np
import pytest

import sum_identity_restate as ir
import sum_restate as sr
from util import GOLDEN

NAMES = ("ka_sum_fam_identity_entries", "ka_sum_fam_identity", "ka_sum_fam_identity_stats")
CASES = sorted(os.path.basename(p)[4:-4] for p in glob.glob(os.path.join(GOLDEN, "idm_*.npz")))
ME = "ka_sum_fam_identity_entries: "


def _entries(first):
    import kalign_amd
    from kalign_amd import api
    L = kalign_amd.load_library()
    first = np.array(first, np.int32)
    n = L.ka_sum_fam_identity_entries(len(first) - 1, api._ptr(first))
    return int(n), L.ka_last_error().decode()


def _rows(name):
    return [r.tobytes() for r in np.load(os.path.join(GOLDEN, "sum_%s.npz" % name))["rows"]]


def test_names_and_version():
    import kalign_amd
    from kalign_amd import api, summary
    L = kalign_amd.load_library()
    for name in NAMES:
        assert name in api.EXPORTS and hasattr(L, name), name
    assert L.ka_abi_version() >= 23
    assert callable(api.FamilySummary.identity) and callable(api.FamilySummary.identity_stats) and callable(api.identity_entries)
    assert callable(summary.pairwise_identity_matrix) and callable(summary.pairwise_identity_matrices)


def test_entries_of_valid_tables():
    assert _entries([0, 1])[0] == 1
    assert _entries([0, 3, 4, 8])[0] == 9 + 1 + 16
    assert _entries([0, 46340])[0] == 46340 * 46340                  # the largest single family: 2 147 395 600 < 2^31
    assert _entries([0, 32768, 65535])[0] == 32768 ** 2 + 32767 ** 2 == 2 ** 31 - 65535
    from kalign_amd import api
    assert api.identity_entries([3, 1, 4]) == 26
    assert api.identity_entries([46340]) == 46340 ** 2


def test_entries_refuses_fam_first():
    for first in ([1, 3, 4, 8], [0, 4, 3, 8]):
        assert _entries(first) == (-1, ME + "fam_first does not ascend from 0 to numseq")
    assert _entries([0, 3, 3, 8]) == (-1, ME + "empty family")
    from kalign_amd import KalignAmdError, api
    with pytest.raises(KalignAmdError, match="ka_sum_fam_identity_entries: empty family"):
        api.identity_entries([3, 0, 5])


def test_entries_refuses_two_to_the_31():
    """sizes alone: nothing is allocated"""
    assert 46341 ** 2 == 2147488281 > 2 ** 31
    assert _entries([0, 46341]) == (-1, ME + "family 0: 46341 rows bring the matrices to 2147488281 entries; a batch holds fewer than 2^31")
    # the sum reaches 2^31 exactly, at the second family
    assert _entries([0, 32768, 65536]) == (-1, ME + "family 1: 32768 rows bring the matrices to 2147483648 entries; a batch holds fewer than 2^31")
    from kalign_amd import KalignAmdError, api
    with pytest.raises(KalignAmdError, match="family 0: 46341 rows bring the matrices to 2147488281 entries"):
        api.identity_entries([46341])


def test_restatement_equals_the_reference():
    assert len(CASES) >= 15 and CASES == sorted(os.path.basename(p)[4:-4] for p in glob.glob(os.path.join(GOLDEN, "sum_*.npz")))
    for name in CASES:
        want = np.load(os.path.join(GOLDEN, "idm_%s.npz" % name))["identity"]
        got, m, c = ir.identity(_rows(name))
        assert got.dtype == np.float64 and got.shape == want.shape and (got == want).all(), name
        assert m.dtype == np.int32 and c.dtype == np.int32
        assert np.array_equal(m, m.T) and np.array_equal(c, c.T) and np.array_equal(got, got.T), name


def test_restatement_sums_equal_the_summary_restatement():
    """over i < j the matches are the family's matching pairs, the compared columns its compared pairs"""
    for name in CASES:
        rows = _rows(name)
        _, m, c = ir.identity(rows)
        s = sr.summary(rows)
        assert ir.upper_sums(m, c) == (s["matching_pairs"], s["compared_pairs"]), name


def test_restatement_rules():
    ident, m, c = ir.identity([b"AC-G", b"----", b"A-TG", b"-C--"])
    assert m.tolist() == [[3, 0, 2, 1], [0, 0, 0, 0], [2, 0, 3, 0], [1, 0, 0, 1]]
    assert c.tolist() == [[3, 0, 2, 1], [0, 0, 0, 0], [2, 0, 3, 0], [1, 0, 0, 1]]
    assert ident.tolist() == [[1.0, 0.0, 1.0, 1.0], [0.0, 1.0, 0.0, 0.0], [1.0, 0.0, 1.0, 0.0], [1.0, 0.0, 0.0, 1.0]]
    ident, m, c = ir.identity([b"Aa.-", b"AA-."], gap=b".")
    assert m.tolist() == [[3, 1], [1, 3]] and c.tolist() == [[3, 2], [2, 3]] and ident[0, 1] == 0.5
