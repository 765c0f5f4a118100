"""The host side of the gap pass of the summary stage: the names and the ABI revision; the numpy restatement
(tests/sum_gap_restate.py) against every golden recorded from the reference's benchmarks/analysis.py: compute_gap_stats
(tests/golden/gap_*.npz for the rows of the sum_ case of the same name, gapx_*.npz with rows of their own), integers and
doubles with ==; and ka_sum_fam_gap_values, the library's one statement of the seven doubles, on the goldens' counts, bit
for bit, the zero-denominator cases included.  No GPU, no tolerance."""
import glob
import os

import numpy as np
import pytest

import sum_gap_restate as gr
from util import GOLDEN

NAMES = ("ka_sum_fam_gaps", "ka_sum_fam_gap_values", "ka_sum_fam_ungapped_size", "ka_sum_fam_ungapped", "ka_sum_fam_gap_stats")
CASES, OWN = gr.golden_names(GOLDEN)


def goldens():
    return gr.goldens(GOLDEN)


def same_bits(x, y):
    return np.float64(x).tobytes() == np.float64(y).tobytes()


def test_names_and_version():
    import kalign_amd
    from kalign_amd import api, summary
    L = kalign_amd.load_library()
    for name in NAMES:
        assert name in api.EXPORTS and hasattr(L, name), name
    assert L.ka_abi_version() >= 26
    for m in ("gaps", "ungapped", "gap_stats"):
        assert callable(getattr(api.FamilySummary, m)), m
    for m in ("gap_stats", "gap_stats_families", "dealign", "dealign_families"):
        assert callable(getattr(summary, m)), m
    assert tuple(api.GAP_COUNTS) == gr.COUNTS and tuple(api.GAP_VALUES) == gr.VALUES


def test_the_cases_are_there():
    assert len(CASES) >= 19 and len(OWN) >= 6
    assert CASES == sorted(os.path.basename(p)[4:-4] for p in glob.glob(os.path.join(GOLDEN, "sum_*.npz")))
    for name, _, want in goldens():
        assert sorted(want) == sorted(gr.FIELDS), name
        for k, v in want.items():
            assert v.shape == () and v.dtype == (np.float64 if k in gr.VALUES else np.int64), (name, k)


def test_restatement_equals_the_reference():
    n = 0
    for name, rows, want in goldens():
        got = gr.gaps(rows)
        for k in gr.FIELDS:
            if k in gr.VALUES:
                assert same_bits(got[k], want[k]), (name, k, got[k], float(want[k]))
            else:
                assert got[k] == int(want[k]), (name, k, got[k], int(want[k]))
        # the row records add up to the family's counts
        rec = got["rows"].astype(np.int64)
        w = got["alignment_length"]
        assert rec[:, 0].sum() == got["characters"] == got["n_seqs"] * w - got["total_gaps"], name
        assert rec[:, 3].sum() == got["n_gap_blocks"] and (rec[:, 1] + rec[:, 2]).sum() == got["terminal_gaps"], name
        assert got["gap_opens_per_seq"] == got["n_gap_blocks"] / got["n_seqs"], name
        n += 1
    assert n >= 19 + 6


def test_gap_values_equal_the_reference_bit_for_bit():
    """the library's doubles from the restatement's counts (which the test above holds to the goldens' integers) against the
    goldens' doubles, one family at a time and all in one call"""
    from kalign_amd import api
    cases = goldens()
    counts = np.stack([gr.counts(rows) for _, rows, _ in cases])
    both = api.gap_values(counts)
    assert both.shape == (len(cases), 7) and both.dtype == np.float64
    for i, (name, rows, want) in enumerate(cases):
        one = api.gap_values(counts[i])
        for j, k in enumerate(gr.VALUES):
            assert same_bits(one[0, j], want[k]) and same_bits(both[i, j], want[k]), (name, k, one[0, j], float(want[k]))
        assert (one[0] == gr.values(counts[i])).all(), name


def test_gap_values_zero_denominators():
    from kalign_amd import api
    z = {name: want for name, _, want in goldens()}
    # every row all-gap: the mean length is 0, so the expansion factor is 0.0; one block per row
    v = api.gap_values([3, 5, 0, 15, 3, 30, 0, 5])[0]
    assert v.tolist() == [0.0, 0.0, 1.0, 5.0, 10.0, 0.0, 1.0]
    assert all(same_bits(v[j], z["x all_allgap"][k]) for j, k in enumerate(gr.VALUES))
    # no gap at all: no block, so the mean block length is 0.0
    v = api.gap_values([2, 7, 14, 0, 0, 0, 0, 0])[0]
    assert v.tolist() == [7.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert all(same_bits(v[j], z["x no_gap"][k]) for j, k in enumerate(gr.VALUES))
    # two roundings: 7 / (10 / 3) is not 21 / 10 rounded once
    v = api.gap_values([3, 7, 10, 11, 4, 5, 6, 2])[0]
    assert v[0] == 10.0 / 3.0 and v[1] == 7.0 / (10.0 / 3.0) and v[3] == 11.0 / 4.0 and v[6] == 2.0 / 7.0
    # counts nothing can hold (no row, no column): 0.0, not a division by zero
    assert api.gap_values([0, 0, 0, 0, 0, 0, 0, 0])[0].tolist() == [0.0] * 7


def test_gap_values_refuses():
    import kalign_amd
    from kalign_amd import api
    L = kalign_amd.load_library()
    c, v = np.zeros(8, np.int64), np.zeros(7, np.float64)
    for args in ((0, api._ptr(c), api._ptr(v)), (1, None, api._ptr(v)), (1, api._ptr(c), None)):
        assert L.ka_sum_fam_gap_values(*args) != 0
        assert L.ka_last_error().decode() == "ka_sum_fam_gap_values: bad arguments"
    assert L.ka_sum_fam_ungapped_size(None) == -1 and L.ka_last_error().decode() == "ka_sum_fam_ungapped_size: bad arguments"
    for call in (lambda: L.ka_sum_fam_gaps(None, None, None, None), lambda: L.ka_sum_fam_ungapped(None, None, 0, None),
                 lambda: L.ka_sum_fam_gap_stats(None, None)):
        assert call() != 0 and L.ka_last_error().decode().endswith(": bad arguments")


def test_restatement_rules():
    """the contract's corner cases by hand"""
    d = gr.gaps([b"--A-C--", b"-------", b"ACGTACG", b"A-----C"])
    assert d["rows"].tolist() == [[2, 2, 2, 3], [0, 7, 7, 1], [7, 0, 0, 0], [2, 0, 0, 1]]
    assert (d["characters"], d["total_gaps"], d["n_gap_blocks"], d["terminal_gaps"], d["internal_gaps"]) == (11, 17, 5, 18, 6)
    assert d["n_gappy_columns"] == 3                              # columns 1, 3 and 5 hold 3 gaps of 4; the others 2: not gappy
    d = gr.gaps([b".-A", b"..-"], gap=b".")
    assert d["rows"].tolist() == [[2, 1, 0, 1], [1, 2, 0, 1]] and d["n_gappy_columns"] == 1
    rows, off = gr.ungapped([b"--A-C--", b"-------", b"ACGTACG"])
    assert rows == [b"AC", b"", b"ACGTACG"] and off.tolist() == [0, 2, 2, 9] and off.dtype == np.int64
    with pytest.raises(ValueError):
        gr.gaps([b"AC", b"A"])
