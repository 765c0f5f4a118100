"""The inputs of the detail tests, without a GPU: the numpy restatement of ka_cmp_fam_detail (tests/detail_restate.py)
against the column correctness recorded from the reference's _column_correctness (tests/golden/col_*.npz) on all 28 stored
pairs and against the counts of the comparison stage's restatement (tests/cmp_restate.py), and the edge batch of
test_gpu_compare_detail.py: that it holds the edges it is made for, and both flag values often enough that a kernel which
writes a constant cannot pass."""
import numpy as np
import pytest

import cmp_restate as R
import detail_cases as D
import detail_restate as DR

NAMES = ("ka_cmp_detail", "ka_cmp_fam_detail", "ka_cmp_detail_stats", "ka_cmp_fam_detail_stats", "ka_calibration")


def test_names_and_version():
    import kalign_amd
    from kalign_amd import api, compare, summary
    L = kalign_amd.load_library()
    for name in NAMES:
        assert name in api.EXPORTS and hasattr(L, name), name
    assert L.ka_abi_version() >= 24
    assert callable(api.Comparer.detail) and callable(api.FamilyComparer.detail)
    assert callable(api.Comparer.detail_stats) and callable(api.FamilyComparer.detail_stats)
    for f in (compare.column_correctness, compare.column_correctness_families, compare.calibration, compare.calibrate_families,
              summary.mask_by_confidence):
        assert callable(f)


@pytest.fixture(scope="module")
def stored():
    """the 28 stored pairs with their restated detail, computed once"""
    pairs = D.stored_pairs()
    assert len(pairs) == 28
    return [(name, k, r, t, flags, DR.detail(r, t)) for name, k, r, t, flags in pairs]


def _consistent(d):
    for side in ("test_columns", "ref_columns"):
        k = d[side]["residues"].astype(np.int64)
        assert np.array_equal(d[side]["correct"] != 0, d[side]["common"] == k * (k - 1)), side


def test_restatement_equals_the_reference(stored):
    for name, k, r, t, flags, d in stored:
        got = d["test_columns"]["correct"]
        assert got.dtype == np.uint8 and got.shape == flags.shape == (len(t[0]),) and np.array_equal(got, flags), (name, k)
        assert np.array_equal(DR.column_flags(r, t), flags), (name, k)
    assert any(f.all() for *_, f, _ in stored) and sum(int((f == 0).sum()) for *_, f, _ in stored) > 1000


def test_flags_follow_from_the_counts(stored):
    for *_, d in stored:
        _consistent(d)


def test_sums_are_the_score_counts(stored):
    """planes 0 / 1 / 2 sum to ref_total_aligned_pairs, test_total_aligned_pairs and identical_aligned; the reference
    flags over the columns with two residues or more sum to tc_correct (every column scored)"""
    for name, k, r, t, _, d in stored:
        c = R.counts(r, t, R.scored_mask(r))
        assert d["res"].sum(axis=0, dtype=np.int64).tolist() == [c[0], c[4], c[2]], (name, k)
        rc = d["ref_columns"]
        two = rc["residues"] >= 2
        assert int(rc["correct"][two].sum()) == c[10] and int(two.sum()) == c[11], (name, k)
        assert int(d["test_columns"]["common"].sum()) == c[2] == int(rc["common"].sum())


@pytest.fixture(scope="module")
def edge():
    refs, tests, notes = D.edge_batch()
    return refs, tests, notes, [DR.detail(r, t) for r, t in zip(refs, tests)]


def test_edge_batch_holds_its_edges(edge):
    refs, tests, notes, want = edge
    sizes = [len(r) for r in refs]
    assert set(sizes) >= set(D.EDGE_N) | set(D.DEEP_N) | {40}
    widths = [(len(r[0]), len(t[0])) for r, t in zip(refs, tests)]
    assert {w for w, _ in widths} >= set(D.EDGE_W) and {w for _, w in widths} >= set(D.EDGE_W)
    assert any(a < b for a, b in widths) and any(a > b for a, b in widths)
    for f in notes["deep"]:
        assert widths[f] == (9, 9) and sizes[f] in D.DEEP_N
    # the deep families take 3 and 5 j-tiles of 32 rows; the 40-row family two by the LDS budget (a row pair of
    # (600 + 616) int16: 26 of them fill 64 KiB)
    assert [-(-sizes[f] // 32) for f in notes["deep"]] == [3, 5]
    (f,) = notes["lds"]
    pad = lambda w: (w + 7) & ~7                                          # noqa: E731
    assert sizes[f] == 40 and widths[f] == (600, 610) and 65536 // ((pad(600) + pad(610)) * 2) == 26 < 32 < 40 <= 2 * 26
    # six consecutive narrow families; with more than 2048 columns in all a wave of the column pass takes two or more
    # consecutive columns, so a chunk spans several of them
    n = notes["narrow"]
    assert n == list(range(n[0], n[0] + 6)) and all(max(widths[f]) <= 3 for f in n) and {1, 2, 3} == {w for f in n for w in widths[f]}
    assert sum(a + b for a, b in widths) > 2048
    (f,) = notes["gap_ref_col"]
    assert (want[f]["ref_columns"]["residues"] == 0).any()
    (f,) = notes["gap_test_col"]
    assert (want[f]["test_columns"]["residues"] == 0).any()
    assert any((want[f]["test_columns"]["residues"] == 0).any() for f in notes["lds"])
    (f,) = notes["no_residues"]
    assert any(not R.is_res(np.frombuffer(row, np.uint8)).any() for row in refs[f])
    assert sorted(sizes[f] for f in notes["near"]) == sorted(D.EDGE_N + D.DEEP_N)
    for d in want:
        _consistent(d)


def test_edge_batch_mixes_both_flag_values(edge):
    """of the columns with two residues or more, a fifth at least is correct and a fifth at least is not, on each side;
    and every family made to be nearly right shows both values"""
    *_, notes, want = edge
    for side in ("test_columns", "ref_columns"):
        flags = np.concatenate([d[side]["correct"][d[side]["residues"] >= 2] for d in want])
        assert len(flags) > 1000
        assert 5 * int(flags.sum()) >= len(flags) and 5 * int((flags == 0).sum()) >= len(flags), (side, int(flags.sum()), len(flags))
    for f in notes["near"]:
        for side in ("test_columns", "ref_columns"):
            two = want[f][side]["correct"][want[f][side]["residues"] >= 2]
            assert two.any() and not two.all(), (f, side)
