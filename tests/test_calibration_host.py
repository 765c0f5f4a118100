"""ka_calibration (host only, no GPU) against the reference's brier_score, expected_calibration_error and
calibration_curve recorded in tests/golden/cal_*.npz, per segment and pooled, and every refusal with its message.

ece, the bin fractions and the bin counts are compared with == (NaN positions equal): they are the reference's operations
in its order.  brier is compared within (n + 2) * 2**-52 relative, which is derived, not measured: the reference squares
through pow(), which may differ from the product in the last bit of a term (one rounding, 2**-52 relative per term), and an
n-term sum of non-negative terms in the same order carries that no further than the sum's own n roundings already allow;
the final division is the same correctly rounded operation on both sides."""
import glob
import os

import numpy as np
import pytest

from util import GOLDEN

CASES = sorted(os.path.basename(p)[4:-4] for p in glob.glob(os.path.join(GOLDEN, "cal_*.npz")))


def _call(seg_first, predicted, actual, n_bins, want=(0, 1, 2, 3)):
    """(rc, message, brier, ece, fraction, counts) of one ka_calibration call; outputs not in `want` are passed as NULL"""
    import kalign_amd
    from kalign_amd import api
    L = kalign_amd.load_library()
    first = np.ascontiguousarray(seg_first, np.int64)
    S = len(first)
    p = np.ascontiguousarray(predicted, np.float64)
    a = np.ascontiguousarray(actual, np.uint8)
    nb = max(n_bins, 1)
    out = [np.full(S, -7.0), np.full(S, -7.0), np.full((S, nb), -7.0), np.full((S, nb), -7, np.int64)]
    ptrs = [api._ptr(o) if k in want else None for k, o in enumerate(out)]
    rc = L.ka_calibration(S - 1, api._ptr(first), api._ptr(p), api._ptr(a), n_bins, *ptrs)
    return (rc, L.ka_last_error().decode() if rc else "", *out)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def test_cases_are_the_ones_asked_for():
    assert set(CASES) >= {"ens_bb11001_r3", "ens_bb30014_r3", "ens_dna40_r3", "random10", "random7", "exact10", "exact7", "onebin",
                          "empty_segment", "no_items"}
    z = np.load(os.path.join(GOLDEN, "cal_random10.npz"))
    assert len(z["seg_first"]) == 29 and np.array_equal(z["predicted"], z["predicted"].astype(np.float32).astype(np.float64))
    z = np.load(os.path.join(GOLDEN, "cal_exact10.npz"))
    assert set(z["predicted"].tolist()) == {0.0, 1.0} | {k / 10 for k in range(1, 10)}
    z = np.load(os.path.join(GOLDEN, "cal_onebin.npz"))
    assert (z["counts"][-1] != 0).sum() == 1
    z = np.load(os.path.join(GOLDEN, "cal_empty_segment.npz"))
    assert (np.diff(z["seg_first"]) == 0).sum() == 3


@pytest.mark.parametrize("name", CASES)
def test_against_the_reference(name):
    z = np.load(os.path.join(GOLDEN, "cal_%s.npz" % name))
    n_bins = int(z["n_bins"])
    rc, msg, brier, ece, frac, counts = _call(z["seg_first"], z["predicted"], z["actual"], n_bins)
    assert rc == 0, msg
    assert _same(ece, z["ece"]) and _same(frac, z["fraction"]) and _same(counts, z["counts"])
    n = np.concatenate([np.diff(z["seg_first"]), [z["seg_first"][-1]]])
    print(name, "brier: largest relative difference", float(np.max(np.abs(brier - z["brier"]) / np.maximum(z["brier"], 1e-300))))
    assert (np.abs(brier - z["brier"]) <= (n + 2) * 2.0 ** -52 * z["brier"]).all()
    # an empty slot: 0.0, 0.0, NaNs and zeros
    for s in np.flatnonzero(n == 0):
        assert brier[s] == 0.0 and ece[s] == 0.0 and np.isnan(frac[s]).all() and not counts[s].any()


def test_python_layer_returns_the_reference_keys():
    from kalign_amd import compare
    z = np.load(os.path.join(GOLDEN, "cal_random7.npz"))
    per, pooled = compare.calibration(z["predicted"], z["actual"], n_bins=7, segments=np.diff(z["seg_first"]))
    assert len(per) == 28
    for s, d in enumerate(per + [pooled]):
        assert sorted(d) == ["bin_centers", "bin_counts", "brier_score", "ece", "fraction_correct"]
        assert d["ece"] == z["ece"][s] and d["bin_counts"] == z["counts"][s].tolist() and d["bin_centers"] == z["centers"].tolist()
        assert _same(np.asarray(d["fraction_correct"]), z["fraction"][s])
    z = np.load(os.path.join(GOLDEN, "cal_onebin.npz"))
    d = compare.calibration(z["predicted"], z["actual"])
    assert d["ece"] == z["ece"][-1] == z["ece"][0] and d["bin_counts"] == z["counts"][-1].tolist()


def test_every_output_is_optional():
    z = np.load(os.path.join(GOLDEN, "cal_exact7.npz"))
    full = _call(z["seg_first"], z["predicted"], z["actual"], 7)
    for k in range(4):
        got = _call(z["seg_first"], z["predicted"], z["actual"], 7, want=(k,))
        assert got[0] == 0
        for q in range(4):
            assert _same(got[2 + q], full[2 + q]) if q == k else (got[2 + q] == -7).all()


def test_refusals_name_the_item_and_write_nothing():
    p, a = [0.25, 0.5, 0.75, 1.0], [0, 1, 1, 0]
    nan = float("nan")
    for args, msg in (
            (([0, 4], p, a, 0), "ka_calibration: n_bins 0 < 1"),
            (([0, 4], p, a, -3), "ka_calibration: n_bins -3 < 1"),
            (([1, 4], p, a, 10), "ka_calibration: seg_first does not ascend from 0 (segment 0 starts at 1)"),
            (([0, 3, 2, 4], p, a, 10), "ka_calibration: seg_first does not ascend from 0 (segment 1 ends before it starts)"),
            (([0, 4], [0.25, 0.5, 1.5, 1.0], a, 10), "ka_calibration: item 2: predicted 1.5 is not in [0, 1]"),
            (([0, 4], [0.25, -0.125, 0.5, 1.0], a, 10), "ka_calibration: item 1: predicted -0.125 is not in [0, 1]"),
            (([0, 2, 4], [0.25, 0.5, 0.75, nan], a, 10), "ka_calibration: item 3: predicted nan is not in [0, 1]"),
            (([0, 4], p, [0, 1, 1, 2], 10), "ka_calibration: item 3: actual 2 is neither 0 nor 1")):
        rc, got, *out = _call(*args)
        assert rc != 0 and got == msg
        assert all((o == -7).all() for o in out), msg
    # items beyond the last segment are not read
    rc, _, brier, *_ = _call([0, 2], [0.25, 0.5, 7.0], [0, 1, 9], 10)
    assert rc == 0 and brier[0] == brier[1] == (0.25 * 0.25 + 0.5 * 0.5) / 2
    from kalign_amd import KalignAmdError, compare
    with pytest.raises(KalignAmdError, match=r"ka_calibration: item 2: predicted 1.5 is not in \[0, 1\]"):
        compare.calibration([0.25, 0.5, 1.5], [0, 1, 1])
    with pytest.raises(KalignAmdError, match="ka_calibration: item 1: actual 3 is neither 0 nor 1"):
        compare.calibration([0.25, 0.5], [0, 3])
    with pytest.raises(KalignAmdError, match="ka_calibration: n_bins 0 < 1"):
        compare.calibration([0.25, 0.5], [0, 1], n_bins=0)
