"""The host side of scoring a batch of families (ka_cmp_fam): ka_cmp_fam_check accepts a valid packed batch and refuses
each broken one with the family's number and the cause the one-family call gives; compare_families pairs every family's
rows as compare() pairs them and names the family in its errors.  No GPU: the check needs no context, and the pairing is
watched through a stand-in for the context."""
import numpy as np
import pytest

FAMS = [["AC-D", "A-CD", "ACD-"], ["GGT-A", "G-TAA"], ["MK--L", "M-K-L", "MKL--", "--MKL"]]


def _check(L, fams, first=None, lens=None, widths=None):
    from kalign_amd import api
    rows, w = api.pack_families(fams)
    ff = api._fam_first([len(f) for f in fams]) if first is None else np.array(first, np.int32)
    ll = api.residue_lens([r for f in fams for r in f]) if lens is None else np.array(lens, np.int32)
    ww = w if widths is None else np.array(widths, np.int32)
    rc = L.ka_cmp_fam_check(len(ff) - 1, api._ptr(ff), api._ptr(ll), api._ptr(rows), api._ptr(ww))
    return rc, L.ka_last_error().decode()


def test_names_and_version():
    import kalign_amd
    from kalign_amd import api, compare
    L = kalign_amd.load_library()
    for name in ("ka_cmp_fam_check", "ka_cmp_fam_create", "ka_cmp_fam_destroy", "ka_cmp_fam_set_masks", "ka_cmp_fam_score", "ka_cmp_fam_stats"):
        assert name in api.EXPORTS and hasattr(L, name), name
    assert L.ka_abi_version() >= 18
    assert hasattr(kalign_amd.Context, "family_comparer") and callable(compare.compare_families)


def test_packed_layout_is_the_batch_hand_out():
    """families in order, the rows of family f alnlen_f + 1 bytes apart"""
    from kalign_amd import api
    rows, w = api.pack_families(FAMS)
    assert w.tolist() == [4, 5, 5] and len(rows) == 3 * 5 + 2 * 6 + 4 * 6
    assert rows[5:9].tobytes() == b"A-CD" and rows[15:20].tobytes() == b"GGT-A" and rows[15 + 12 + 6:15 + 12 + 11].tobytes() == b"M-K-L"


def test_check_accepts_a_valid_batch():
    import kalign_amd
    L = kalign_amd.load_library()
    assert _check(L, FAMS)[0] == 0
    # a sequence without residues is accepted, as ka_cmp_create accepts it for a family alone
    assert _check(L, [["AC-D", "----", "ACD-"], FAMS[1]])[0] == 0


def test_check_refuses_fam_first():
    import kalign_amd
    L = kalign_amd.load_library()
    for first in ([1, 3, 5, 9], [0, 5, 3, 9]):
        rc, msg = _check(L, FAMS, first=first)
        assert rc != 0 and msg == "ka_cmp_fam_check: fam_first does not ascend from 0 to numseq"
    rc, msg = _check(L, FAMS, first=[0, 3, 3, 9])
    assert rc != 0 and msg == "ka_cmp_fam_check: empty family"


def test_check_refuses_a_family_of_one():
    import kalign_amd
    L = kalign_amd.load_library()
    rc, msg = _check(L, [FAMS[0], ["ACGT-"], FAMS[2]])
    assert rc != 0 and msg == "ka_cmp_fam_check: family 1: 1 sequences; a comparison needs two at least"


def test_check_refuses_a_letter_count():
    import kalign_amd
    from kalign_amd import api
    L = kalign_amd.load_library()
    lens = api.residue_lens([r for f in FAMS for r in f])
    lens[6] += 1                                                  # family 2, its row 1
    rc, msg = _check(L, FAMS, lens=lens)
    assert rc != 0 and msg == ("ka_cmp_fam_check: family 2: row 1 holds 3 letters, its sequence 4 "
                               "(every alignment must hold the same sequences)")


def test_check_refuses_a_long_sequence():
    import kalign_amd
    L = kalign_amd.load_library()
    long_ = "A" * 32768 + "-"
    rc, msg = _check(L, [FAMS[0], ["ACGT" + "-" * 32765, long_]])
    assert rc != 0 and msg == "ka_cmp_fam_check: family 1: sequence 1 has 32768 residues; the position maps hold at most 32767"
    assert _check(L, [FAMS[0], ["ACGT" + "-" * 32764, long_[1:]]])[0] == 0      # 32767 is the limit itself


def test_check_refuses_a_width():
    import kalign_amd
    L = kalign_amd.load_library()
    rc, msg = _check(L, FAMS, widths=[4, 0, 5])
    assert rc != 0 and msg == "ka_cmp_fam_check: family 1: alignment width 0 does not fit row stride 1"


class _Ctx:
    """what compare_families asks of a context: the rows it hands over are kept"""

    def __init__(self):
        self.refs = self.tests = None
        self.closed = False

    def family_comparer(self, refs):
        self.refs = refs
        return self

    def score(self, tests, max_gap_frac=-1.0, column_masks=None):
        self.tests, self.rule = tests, (max_gap_frac, column_masks)
        return ["r%d" % k for k in range(len(tests))]

    def close(self):
        self.closed = True


def test_compare_families_pairs_by_name_as_compare():
    from kalign_amd import compare as kc
    names = ["zeta", "alpha", "mid"]
    ref = list(zip(names, FAMS[0]))
    test_rows = ["ACD-", "AC-D", "A-CD"]
    perm = [2, 0, 1]
    test = [(names[k], test_rows[k]) for k in perm]
    c = _Ctx()
    out = kc.compare_families(c, [ref, FAMS[1], dict(ref)], [test, FAMS[1], dict(test)], max_gap_frac=0.2, column_masks=[None, [1] * 5, None])
    assert out == ["r0", "r1", "r2"] and c.closed and c.rule == (0.2, [None, [1] * 5, None])
    want = kc.pair_rows(ref, test)
    assert (c.refs[0], c.tests[0]) == want == (c.refs[2], c.tests[2])
    assert want[0] == [b"A-CD", b"ACD-", b"AC-D"] and want[1] == [b"AC-D", b"A-CD", b"ACD-"]      # alpha, mid, zeta
    assert (c.refs[1], c.tests[1]) == ([r.encode() for r in FAMS[1]],) * 2                         # unnamed: by position


def test_compare_families_errors_name_the_family():
    from kalign_amd import KalignAmdError
    from kalign_amd import compare as kc
    good = [("a", "AC-D"), ("b", "A-CD")]
    c = _Ctx()
    with pytest.raises(KalignAmdError, match=r"family 1: the alignments do not hold the same names \('b' is in one only\)"):
        kc.compare_families(c, [good, good], [good, [("a", "AC-D"), ("c", "A-CD")]])
    with pytest.raises(KalignAmdError, match=r"family 2: .*the name 'a' occurs twice"):
        kc.compare_families(c, [good, good, good], [good, good, [("a", "AC-D"), ("a", "A-CD")]])
    with pytest.raises(KalignAmdError, match=r"family 0: one alignment has names and the other has none"):
        kc.compare_families(c, [good], [["AC-D", "A-CD"]])
    with pytest.raises(KalignAmdError, match=r"family 1: the reference has 2 sequences, the test alignment 3"):
        kc.compare_families(c, [good, ["AC-D", "A-CD"]], [good, ["AC-D", "A-CD", "ACD-"]])
    with pytest.raises(KalignAmdError, match="2 reference alignments, 1 test alignments"):
        kc.compare_families(c, [good, good], [good])
    assert c.refs is None                                         # nothing reached the device
