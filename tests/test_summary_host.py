"""The host side of the summary stage (ka_sum_fam): the names and the ABI revision, ka_sum_fam_check on valid and broken
packed batches, the numpy restatement (tests/sum_restate.py) against every golden recorded from python-kalign's
kalign.utils (tests/golden/sum_*.npz: floats with ==, strings byte for byte), and the argument checks and packing of the
Python fronts (kalign_amd.summary) watched through a stand-in for the context.  No GPU."""
import glob
import os

import numpy as np
import pytest

import sum_restate as sr
from util import GOLDEN

FAMS = [["AC-D", "A-CD", "ACD-"], ["GGT-A"], ["MK--L", "-----", "MKL--", "--MKL"]]
NAMES = ("ka_sum_fam_check", "ka_sum_fam_create", "ka_sum_fam_destroy", "ka_sum_fam_columns", "ka_sum_fam_summary", "ka_sum_fam_consensus",
         "ka_sum_fam_keep", "ka_sum_fam_compact", "ka_sum_fam_rows_size", "ka_sum_fam_rows", "ka_sum_fam_stats")
CASES = sorted(os.path.basename(p)[4:-4] for p in glob.glob(os.path.join(GOLDEN, "sum_*.npz")))


def _check(L, fams, first=None, widths=None):
    from kalign_amd import api
    rows, w = api.pack_families(fams)
    ff = api._fam_first([len(f) for f in fams]) if first is None else np.array(first, np.int32)
    ww = w if widths is None else np.array(widths, np.int32)
    rc = L.ka_sum_fam_check(len(ff) - 1, api._ptr(ff), api._ptr(rows), api._ptr(ww))
    return rc, L.ka_last_error().decode()


def test_names_and_version():
    import kalign_amd
    from kalign_amd import api, summary
    L = kalign_amd.load_library()
    for name in NAMES:
        assert name in api.EXPORTS and hasattr(L, name), name
    assert L.ka_abi_version() >= 20
    assert hasattr(kalign_amd.Context, "family_summary")
    for name in ("alignment_stats", "consensus_sequence", "remove_gap_columns", "trim_alignment", "alignment_stats_families",
                 "consensus_sequences", "remove_gap_columns_families"):
        assert callable(getattr(summary, name)), name


def test_check_accepts_a_valid_batch():
    """a family of one row and an all-gap row among them; any byte is allowed in a row"""
    import kalign_amd
    L = kalign_amd.load_library()
    assert _check(L, FAMS)[0] == 0
    assert _check(L, [[b"\x01\x80\xff.*-"], ["-"]])[0] == 0


def test_check_refuses_fam_first():
    import kalign_amd
    L = kalign_amd.load_library()
    for first in ([1, 3, 4, 8], [0, 4, 3, 8]):
        rc, msg = _check(L, FAMS, first=first)
        assert rc != 0 and msg == "ka_sum_fam_check: fam_first does not ascend from 0 to numseq"
    rc, msg = _check(L, FAMS, first=[0, 3, 3, 8])
    assert rc != 0 and msg == "ka_sum_fam_check: empty family"


def test_check_refuses_a_width():
    import kalign_amd
    L = kalign_amd.load_library()
    rc, msg = _check(L, FAMS + [["AC"]], widths=[4, 5, 5, 0])
    assert rc != 0 and msg == "ka_sum_fam_check: family 3: alnlen 0"
    rc, msg = _check(L, FAMS, widths=[4, -2, 5])
    assert rc != 0 and msg == "ka_sum_fam_check: family 1: alnlen -2"


def test_check_refuses_too_many_cells():
    """n_f * alnlens[f] stays below 2^31 (the rows themselves are not read by the size checks)"""
    import kalign_amd
    from kalign_amd import api
    L = kalign_amd.load_library()
    first = np.array([0, 3, 3 + 70000], np.int32)
    widths = np.array([4, 40000], np.int32)
    rc = L.ka_sum_fam_check(2, api._ptr(first), api._ptr(np.zeros(16, np.uint8)), api._ptr(widths))
    assert rc != 0 and L.ka_last_error().decode() == "ka_sum_fam_check: family 1: 70000 rows of 40000 columns; a family holds fewer than 2^31 cells"


def _golden(name):
    return np.load(os.path.join(GOLDEN, "sum_%s.npz" % name))


def _blocks(buf, n, widths):
    """the n rows of every block of a golden's back-to-back rows"""
    out, o = [], 0
    for w in widths:
        w = int(w)
        out.append([buf[o + r * w:o + (r + 1) * w].tobytes() for r in range(n)])
        o += n * w
    assert o == len(buf)
    return out


def golden_trims(z):
    return [(None if z["trim_none"][k, 0] else int(z["trim_arg"][k, 0]), None if z["trim_none"][k, 1] else int(z["trim_arg"][k, 1]))
            for k in range(len(z["trim_w"]))]


def test_goldens_are_there():
    assert len(CASES) >= 15 and {"ties", "bytes", "one_row", "allgap_col_row", "dna_only", "dna_one_x"} <= set(CASES)
    for p in glob.glob(os.path.join(GOLDEN, "sum_*.npz")):
        assert os.path.getsize(p) < 100 * 1000, p


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference(name):
    from kalign_amd import summary
    z = _golden(name)
    rows = [r.tobytes() for r in z["rows"]]
    n = len(rows)
    s = sr.summary(rows)
    assert [s["length"], s["n_sequences"]] == z["stats_i"].tolist()
    for k, key in enumerate(("gap_fraction", "conservation", "identity")):
        assert s[key] == z["stats_f"][k], (key, s[key], z["stats_f"][k])
    for t, want in zip(z["cons_thr"], z["cons"]):
        assert sr.consensus(rows, float(t)) == want.tobytes(), t
    for t, want in zip(z["rg_thr"], _blocks(z["rg"], n, z["rg_w"])):
        assert sr.compact(rows, float(t)) == want, t
    w = len(rows[0])
    for (s0, e0), want in zip(golden_trims(z), _blocks(z["trim"], n, z["trim_w"])):
        a, b = summary.trim_range(w, s0, e0)
        assert sr.compact(rows, mask=[a <= c < b for c in range(w)]) == want, (s0, e0)


def test_restatement_ties_and_characters():
    """the tie rule and the byte rule of the restatement on their own, by hand (a check of the oracle, not of the stage),
    and its dicts under the names the stage's Python side gives its outputs"""
    from kalign_amd import api
    d = sr.summary(["AC-", "A-C"])
    assert list(d) == ["length", "n_sequences", "gap_fraction", "conservation", "identity"] + api.SUM_COUNTS
    assert [d[k] for k in api.SUM_COUNTS] == [2, 6, 3, 3, 1, 1]
    c = sr.columns(["QQ-", "RA-", "SA-", "Aa-", "AB-", "BB-", "Ba-", "C.-", "C*-"])
    assert c["top_char"].tobytes() == b"AA-" and c["top_count"].tolist() == [2, 2, 0] and c["n_distinct"].tolist() == [6, 6, 0]
    assert c["same_pairs"].tolist() == [3, 3, 0] and c["n_gap"].tolist() == [0, 0, 9]
    c = sr.columns(["Q", "C", "B", "A", "A", "B", "C"])
    assert c["top_char"].tobytes() == b"C"                        # first seen in row 1, before B and A
    assert sr.ambiguous(["acgu-N", "TTTTTT"]) == b"N" and sr.ambiguous(["acgu-N", "TTTT.T"]) == b"X"
    assert sr.ambiguous(["AC#T"], gap=b"#") == b"N" and sr.ambiguous(["AC-T"], gap=b"#") == b"X"


class _Summary:
    """what the fronts ask of a FamilySummary: answers from the restatement, the arguments kept"""

    def __init__(self, ctx, fams, gap):
        self.ctx, self.fams, self.gap = ctx, fams, gap

    def summary(self):
        return [sr.summary(f, self.gap) for f in self.fams]

    def consensus(self, threshold=0.5):
        self.ctx.rule = ("consensus", threshold)
        t = threshold if hasattr(threshold, "__len__") else [threshold] * len(self.fams)
        return [sr.consensus(f, x, self.gap) for f, x in zip(self.fams, t)]

    def compact(self, gap_threshold=1.0, column_masks=None):
        self.ctx.rule = ("compact", gap_threshold, column_masks)
        t = gap_threshold if hasattr(gap_threshold, "__len__") else [gap_threshold] * len(self.fams)
        m = column_masks or [None] * len(self.fams)
        return [sr.compact(f, x, k, self.gap) for f, x, k in zip(self.fams, t, m)]

    def close(self):
        self.ctx.closed += 1


class _Ctx:
    def __init__(self):
        self.fams = self.rule = None
        self.opened = self.closed = 0

    def family_summary(self, families_rows, gap=b"-"):
        self.fams = families_rows
        self.opened += 1
        return _Summary(self, families_rows, gap)


def test_fronts_return_the_reference_shapes():
    from kalign_amd import summary
    c = _Ctx()
    z = _golden("ties")
    aln = [r.tobytes().decode("latin-1") for r in z["rows"]]
    st = summary.alignment_stats(c, aln)
    assert list(st) == ["length", "n_sequences", "gap_fraction", "conservation", "identity"]
    assert [st["gap_fraction"], st["conservation"], st["identity"]] == z["stats_f"].tolist()
    assert c.fams == [[r.tobytes() for r in z["rows"]]] and c.opened == c.closed == 1
    for t, want in zip(z["cons_thr"], z["cons"]):
        got = summary.consensus_sequence(c, aln, float(t))
        assert isinstance(got, str) and got == want.tobytes().decode("latin-1")
    for t, want in zip(z["rg_thr"], _blocks(z["rg"], len(aln), z["rg_w"])):
        got = summary.remove_gap_columns(c, aln, float(t))
        assert got == [r.decode("latin-1") for r in want] and c.rule == ("compact", float(t), None)
    for (s0, e0), want in zip(golden_trims(z), _blocks(z["trim"], len(aln), z["trim_w"])):
        assert summary.trim_alignment(c, aln, s0, e0) == [r.decode("latin-1") for r in want]
    assert c.opened == c.closed
    # a list of families: one handle, one threshold or one per family
    fams = [aln, FAMS[0], FAMS[2]]
    n = c.opened
    assert summary.consensus_sequences(c, fams, [0.0, 0.5, 1.0]) == [sr.consensus(f, t).decode() for f, t in zip(fams, [0.0, 0.5, 1.0])]
    assert c.rule == ("consensus", [0.0, 0.5, 1.0]) and c.opened == n + 1
    assert summary.remove_gap_columns_families(c, fams, 0.5) == [[r.decode() for r in sr.compact(f, 0.5)] for f in fams]
    assert [d["identity"] for d in summary.alignment_stats_families(c, fams)] == [sr.summary(f)["identity"] for f in fams]
    assert summary.remove_gap_columns(c, ["--", "--"]) == ["", ""]


def test_trim_is_a_mask_with_the_reference_range_rules():
    from kalign_amd import summary
    c = _Ctx()
    aln = ["ATCGATCG", "ATCGATCG"]
    assert summary.trim_alignment(c, aln, start=2, end=6) == ["CGAT", "CGAT"]
    assert c.rule == ("compact", 1.0, [[0, 0, 1, 1, 1, 1, 0, 0]])
    assert summary.trim_alignment(c, aln, -3) == ["TCG", "TCG"] and summary.trim_alignment(c, aln, None, -6) == ["AT", "AT"]
    assert summary.trim_alignment(c, aln, -100, 1) == ["A", "A"] and summary.trim_alignment(c, aln, 7, 100) == ["G", "G"]
    n = c.opened
    for s0, e0 in ((3, 3), (5, 2), (0, -8), (8, None), (-1, -1)):
        with pytest.raises(ValueError, match="Start position must be less than end position"):
            summary.trim_alignment(c, aln, s0, e0)
    assert c.opened == n                                          # nothing reached the device


def test_fronts_refuse_as_the_reference_does():
    from kalign_amd import summary
    c = _Ctx()
    aln = ["AC-D", "A-CD"]
    for bad in (-0.01, 1.01, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="Threshold must be between 0 and 1"):
            summary.consensus_sequence(c, aln, bad)
        with pytest.raises(ValueError, match="Threshold must be between 0 and 1"):
            summary.remove_gap_columns(c, aln, bad)
        with pytest.raises(ValueError, match="Threshold must be between 0 and 1"):
            summary.consensus_sequences(c, [aln, aln], [0.5, bad])
    with pytest.raises(ValueError, match="2 thresholds for 3 alignments"):
        summary.remove_gap_columns_families(c, [aln, aln, aln], [0.5, 0.5])
    for f in (summary.alignment_stats, summary.consensus_sequence, summary.remove_gap_columns, summary.trim_alignment):
        with pytest.raises(ValueError, match="Empty alignment provided"):
            f(c, [])
        with pytest.raises(ValueError, match="All sequences in alignment must have the same length"):
            f(c, ["ACD", "AC"])
    assert c.opened == 0                                          # nothing reached the device


def test_pack_masks_layout():
    """masks back to back in family order, -1 where a family has none: what ka_sum_fam_keep and ka_cmp_fam_set_masks take"""
    from kalign_amd import KalignAmdError, api
    masks, off = api.pack_masks([None, [1, 0, 2], None, [0, 0]], [4, 3, 5, 2])
    assert masks.tolist() == [1, 0, 2, 0, 0] and masks.dtype == np.int32 and off.tolist() == [-1, 0, -1, 3] and off.dtype == np.int64
    assert api.pack_masks(None, [4, 3]) == (None, None)
    masks, off = api.pack_masks([None, None], [4, 3])
    assert masks is None and off.tolist() == [-1, -1]
    with pytest.raises(KalignAmdError, match="family 1: mask length 2 != alignment length 3"):
        api.pack_masks([None, [1, 0]], [4, 3])
    with pytest.raises(KalignAmdError, match="1 column masks for 2 families"):
        api.pack_masks([None], [4, 3])
