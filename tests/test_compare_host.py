"""CPU: the alignment comparison's host side -- pairing named rows the way the reference does (kalign_amd.compare), its
argument checks, and the stored reference outputs (tests/golden/cmp_*.npz) against the numpy restatement of the
counters (cmp_restate.py) that the GPU tests also use."""
import glob
import os

import numpy as np
import pytest

import cmp_restate as R
from kalign_amd import KalignAmdError
from kalign_amd import compare as kc
from util import GOLDEN

CASES = sorted(os.path.basename(f)[4:-4] for f in glob.glob(os.path.join(GOLDEN, "cmp_*.npz")))


def test_pairs_by_sorted_name():
    r, t = kc.pair_rows([("b", "A-C"), ("a", "CC-"), ("c", "-GG")], {"c": "G-G", "a": "-CC", "b": "AC-"})
    assert r == [b"CC-", b"A-C", b"-GG"] and t == [b"-CC", b"AC-", b"G-G"]


def test_byte_order_of_names():
    # strncmp order: upper case before lower case, "s10" before "s2"
    r, _ = kc.pair_rows([("s2", "A-"), ("s10", "C-"), ("S3", "G-")], [("s10", "-C"), ("S3", "-G"), ("s2", "-A")])
    assert r == [b"G-", b"C-", b"A-"]


def test_unnamed_rows_pair_by_position():
    r, t = kc.pair_rows(["A-C", "CC-"], [b"AC-", b"-CC"])
    assert r == [b"A-C", b"CC-"] and t == [b"AC-", b"-CC"]


@pytest.mark.parametrize("ref,test", [
    ([("a", "A-"), ("a", "C-")], [("a", "A-"), ("b", "C-")]),      # duplicated name in the reference
    ([("a", "A-"), ("b", "C-")], [("b", "A-"), ("b", "C-")]),      # ... in the test
    ([("a", "A-"), ("b", "C-")], [("a", "A-"), ("c", "C-")]),      # a name missing from one
    ([("a", "A-"), ("b", "C-")], [("a", "A-")]),                   # row counts differ
    ([("a", "A-"), ("b", "C-")], ["A-", "C-"]),                    # names on one side only
    (["A-", "C-", "G-"], ["A-", "C-"]),
])
def test_pairing_errors(ref, test):
    with pytest.raises(KalignAmdError):
        kc.pair_rows(ref, test)


def test_float_gap_fraction_rule():
    rows = ["AAAAA-", "AAAA--", "AAA---", "AA----", "A-----"]
    # gaps per column 0..4 and 5 of 5 rows; 1 / 5 <= 0.2f in float
    assert R.scored_mask(rows, 0.2).tolist() == [True, True, False, False, False, False]
    assert R.scored_mask(rows, -1.0).all()
    assert R.scored_mask(rows, 1.0).all()
    assert R.scored_mask(rows, 0.0).tolist() == [True, False, False, False, False, False]


@pytest.mark.parametrize("name", CASES)
def test_golden_restated(name):
    """the reference's stored outputs are what the counters' restatement gives, bit for bit"""
    z = np.load(os.path.join(GOLDEN, "cmp_%s.npz" % name))
    names = [str(n) for n in z["names"]]
    ref = [str(r) for r in z["ref"]]
    tnames = [str(n) for n in z["test_names"]] if "test_names" in z.files else names
    for k, t in enumerate(z["tests"]):
        rr, tt = kc.pair_rows(list(zip(names, ref)), list(zip(tnames, [str(r) for r in t])))
        rr, tt = [x.decode() for x in rr], [x.decode() for x in tt]
        for q, fr in enumerate(z["fracs"]):
            c = R.counts(rr, tt, R.scored_mask(rr, fr))
            sp, rc, pr, f1, tc = R.scores(c)
            assert sp == z["sp"][k]
            assert (rc, pr, f1, tc) == tuple(float(x) for x in z["poar"][k, q])
            assert (c[6], c[7], c[8]) == tuple(int(x) for x in z["poar_i"][k, q])
        c = R.counts(rr, tt, R.scored_mask(rr, column_mask=z["mask"]))
        assert R.scores(c)[1:] == tuple(float(x) for x in z["mask_poar"][k])
        assert (c[6], c[7], c[8]) == tuple(int(x) for x in z["mask_i"][k])


def test_comparer_exported():
    from kalign_amd import api
    assert hasattr(api.Context, "comparer") and "ka_cmp_score_batch" in api.EXPORTS
