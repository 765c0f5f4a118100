"""GPU: where a test alignment agrees with its reference, per residue and per column, for a batch of families in one pass
(ka_cmp_detail, ka_cmp_fam_detail; Comparer.detail, FamilyComparer.detail; kalign_amd.compare.column_correctness*,
calibrate_families; kalign_amd.summary.mask_by_confidence) -- against the column correctness recorded from the
reference (tests/golden/col_*.npz), the numpy restatement of every output (tests/detail_restate.py) on the stored pairs
and on the edge batch of tests/detail_cases.py, the one-family handle, and the score call's counts.  Every value is
compared with ==."""
import os

import numpy as np
import pytest

import cmp_restate as R
import detail_cases as D
import detail_restate as DR
from util import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import kalign_amd
    c = kalign_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def edge():
    """(refs, tests, notes, the restated detail of every family), left unchanged"""
    refs, tests, notes = D.edge_batch()
    return refs, tests, notes, [DR.detail(r, t) for r, t in zip(refs, tests)]


# ---- 1. the stored pairs as one batch ----
def test_stored_pairs_as_one_batch(ctx):
    pairs = D.stored_pairs()
    assert len(pairs) == 28
    cmp = ctx.family_comparer([r for _, _, r, _, _ in pairs])
    got = cmp.detail([t for _, _, _, t, _ in pairs])
    st = cmp.detail_stats()
    cmp.close()
    assert len(got) == 28
    for g, (name, k, r, t, flags) in zip(got, pairs):
        assert g["test_columns"]["correct"].dtype == np.uint8 and np.array_equal(g["test_columns"]["correct"], flags), (name, k)
        assert DR.same(g, DR.detail(r, t)), (name, k)
    assert st["maps_ms"] > 0 and st["walk_ms"] > 0 and st["columns_ms"] > 0 and st["syncs"] == 1


# ---- 2. the edge batch ----
def test_edge_batch_against_the_restatement(ctx, edge):
    refs, tests, _, want = edge
    cmp = ctx.family_comparer(refs)
    got = cmp.detail(tests)
    cmp.close()
    for f, (g, w) in enumerate(zip(got, want)):
        assert DR.same(g, w), (f, len(refs[f]), len(refs[f][0]), len(tests[f][0]))


# ---- 3. one family alone ----
def test_each_family_alone_equals_its_slice(ctx, edge):
    refs, tests, _, want = edge
    for f, (r, t) in enumerate(zip(refs, tests)):
        c = ctx.comparer(r)
        assert c.detail_stats() == dict(maps_ms=0.0, walk_ms=0.0, columns_ms=0.0, launches=0, syncs=0)
        assert DR.same(c.detail(t), want[f]), f
        assert c.detail_stats()["launches"] == 3 and c.detail_stats()["syncs"] == 1
        c.close()


# ---- 4. score, detail, score on one handle ----
def test_detail_between_scores_changes_nothing(ctx, edge):
    from kalign_amd.api import CMP_COUNTS
    refs, tests, _, _ = edge
    rng = np.random.RandomState(7)
    masks = [(rng.rand(len(r[0])) < 0.6).astype(np.int32) if f % 2 else None for f, r in enumerate(refs)]
    plain = ctx.family_comparer(refs)
    want_all, want_masked = plain.score(tests), plain.score(tests, max_gap_frac=0.5, column_masks=masks)
    plain.close()
    cmp = ctx.family_comparer(refs)
    first = cmp.score(tests)
    got = cmp.detail(tests)
    masked = cmp.score(tests, max_gap_frac=0.5, column_masks=masks)
    again = cmp.detail(tests)                                    # (the rule set by the last score plays no part)
    cmp.close()
    assert first == want_all and masked == want_masked
    for f, (g, s, m) in enumerate(zip(got, first, masked)):
        assert DR.same(g, again[f])
        sums = g["res"].sum(axis=0, dtype=np.int64).tolist()
        assert sums == [s["ref_total_aligned_pairs"], s["test_total_aligned_pairs"], s["identical_aligned"]], f
        assert int(g["test_columns"]["common"].sum()) == s["identical_aligned"] == int(g["ref_columns"]["common"].sum())
        rc = g["ref_columns"]
        for sc, scored in ((s, R.scored_mask(refs[f])), (m, R.scored_mask(refs[f], 0.5, masks[f]))):
            counted = scored & (rc["residues"] >= 2)
            assert int(rc["correct"][counted].sum()) == sc["tc_correct"] and int(counted.sum()) == sc["tc_total"], f
    assert all(k in first[0] for k in CMP_COUNTS)


# ---- 5. a refused batch ----
def test_a_refused_batch_launches_nothing(ctx, edge):
    from kalign_amd import KalignAmdError
    refs, tests, _, want = edge
    refs, tests, want = refs[:8], tests[:8], want[:8]
    cmp = ctx.family_comparer(refs)
    zeros = dict(maps_ms=0.0, walk_ms=0.0, columns_ms=0.0, launches=0, syncs=0)
    assert cmp.detail_stats() == zeros
    assert DR.same(cmp.detail(tests)[5], want[5]) and cmp.detail_stats()["launches"] > 0
    bad = list(tests)
    b = next(f for f in range(8) if b"-" in tests[f][1])
    row = bytearray(bad[b][1])
    row[row.index(b"-")] = ord("A")                               # a letter too many
    bad[b] = [bad[b][0], bytes(row)] + bad[b][2:]
    with pytest.raises(KalignAmdError, match=r"ka_cmp_fam_detail: family %d: row 1 holds \d+ letters, its sequence \d+ \(every alignment" % b):
        cmp.detail(bad)
    assert cmp.detail_stats() == zeros
    with pytest.raises(KalignAmdError, match="family 2: the test alignment has 1 rows, the reference"):
        cmp.detail(tests[:2] + [tests[2][:1]] + tests[3:])
    got = cmp.detail(tests)
    assert all(DR.same(g, w) for g, w in zip(got, want)) and cmp.detail_stats()["launches"] > 0
    cmp.close()
    one = ctx.comparer(refs[b])
    with pytest.raises(KalignAmdError, match=r"ka_cmp_detail: row 1 holds \d+ letters, its sequence \d+"):
        one.detail(bad[b])
    assert one.detail_stats() == zeros and DR.same(one.detail(tests[b]), want[b])
    one.close()


# ---- 6. every output pointer is optional ----
def test_every_output_null_but_one(ctx, edge):
    refs, tests, _, want = edge
    refs, tests, want = refs[-12:], tests[-12:], want[-12:]
    keys = [("res", None), ("test_columns", "residues"), ("test_columns", "common"), ("test_columns", "correct"),
            ("ref_columns", "residues"), ("ref_columns", "common"), ("ref_columns", "correct")]
    cmp = ctx.family_comparer(refs)
    for k in range(7):
        got = cmp.detail(tests, want=(k,))
        for q, (a, b) in enumerate(keys):
            for g, w in zip(got, want):
                x, y = (g[a], w[a]) if b is None else (g[a][b], w[a][b])
                assert np.array_equal(x, y) if q == k else not x.any(), (k, q)
    assert cmp.detail(tests, want=())[0]["res"].sum() == 0
    cmp.close()


# ---- 7. launches and synchronisations do not grow with the batch ----
def test_launches_do_not_grow_with_the_batch(ctx, edge):
    """the test maps, the detailed walk once per LDS class in use and the column pass.  Every family of the edge batch
    but the 40 x 600 / 610 one stages less than 16 KiB per tile (one class); that family alone adds the class of its
    tiles, however many families stand beside it"""
    refs, tests, notes, _ = edge
    (big,) = notes["lds"]
    small = [f for f in range(len(refs)) if f != big]

    def stats(fams, times=1):
        cmp = ctx.family_comparer([refs[f] for f in fams] * times)
        cmp.detail([tests[f] for f in fams] * times)
        st = cmp.detail_stats()
        cmp.close()
        return st["launches"], st["syncs"]

    one = stats(small[:1])
    assert one == (3, 1)
    assert stats(small) == one and stats([big]) == one
    whole = stats(range(len(refs)))
    assert whole == (4, 1) and stats(range(len(refs)), times=3) == whole


# ---- 8. the Python layer ----
def test_column_correctness_families_pairs_rows_by_name(ctx):
    from kalign_amd import compare as kc
    pairs = D.stored_pairs()
    z = np.load(os.path.join(GOLDEN, "cmp_syn_shuffled.npz"))
    names, tnames = [str(n) for n in z["names"]], [str(n) for n in z["test_names"]]
    assert names != tnames
    refs = [list(zip(names, (str(x) for x in z["ref"])))] + [r for _, _, r, _, _ in pairs[:6]]
    tests = [list(zip(tnames, (str(x) for x in z["tests"][0])))] + [t for _, _, _, t, _ in pairs[:6]]
    got = kc.column_correctness_families(ctx, refs, tests)
    want = [np.load(os.path.join(GOLDEN, "col_syn_shuffled.npz"))["correct"][0]] + [f for *_, f in pairs[:6]]
    assert len(got) == 7 and all(np.array_equal(g, w) for g, w in zip(got, want))
    assert np.array_equal(kc.column_correctness(ctx, refs[0], tests[0]), want[0])


def test_calibrate_families_against_the_reference(ctx):
    """the real ensembles' stored column confidences against the correctness of their rows versus member 0: the flags and
    the metrics of tests/golden/cal_ens_*.npz, per family; the pool against the restated reference arithmetic"""
    from kalign_amd import compare as kc
    srcs = ("bb11001_r3", "bb30014_r3", "dna40_r3")
    cal = [np.load(os.path.join(GOLDEN, "cal_ens_%s.npz" % s)) for s in srcs]
    ens = [np.load(os.path.join(GOLDEN, "ens_real_%s.npz" % s)) for s in srcs]
    refs = [[str(r) for r in z["members"][0]] for z in ens]
    tests = [[str(r) for r in z["ens_rows"]] for z in ens]
    out = kc.calibrate_families(ctx, refs, tests, [z["ens_col_conf"] for z in ens], n_bins=10)
    for f, (d, z) in enumerate(zip(out["families"], cal)):
        assert np.array_equal(out["correct"][f], z["actual"])
        assert d["ece"] == z["ece"][0] and d["bin_counts"] == z["counts"][0].tolist()
        assert np.array_equal(np.asarray(d["fraction_correct"]), z["fraction"][0], equal_nan=True)
        n = len(z["actual"])
        assert abs(d["brier_score"] - z["brier"][0]) <= (n + 2) * 2.0 ** -52 * z["brier"][0]
    pooled = kc.calibration(np.concatenate([z["predicted"] for z in cal]), np.concatenate([z["actual"] for z in cal]))
    assert sorted(out["pooled"]) == sorted(pooled)
    for k in pooled:                                             # (an empty bin's fraction is NaN)
        assert np.array_equal(np.asarray(out["pooled"][k]), np.asarray(pooled[k]), equal_nan=True), k
    assert sum(pooled["bin_counts"]) == sum(len(z["actual"]) for z in cal)


def test_mask_by_confidence_against_the_reference(ctx):
    from kalign_amd import summary
    srcs = ("bb11001_r3", "bb30014_r3", "dna40_r3")
    cal = [np.load(os.path.join(GOLDEN, "cal_ens_%s.npz" % s)) for s in srcs]
    fams = [[bytes(r).decode("latin-1") for r in z["rows"]] for z in cal]
    thr = [z["mask_thr"] for z in cal]
    assert all(len(t) == len(thr[0]) for t in thr)
    for q in range(len(thr[0])):
        if len({float(t[q]) for t in thr}) == 1:
            got = summary.mask_by_confidence(ctx, fams, [z["conf"] for z in cal], float(thr[0][q]))
        else:                                                    # (a threshold taken from the family's own values)
            got = [summary.mask_by_confidence(ctx, [fam], [z["conf"]], float(t[q]))[0] for fam, z, t in zip(fams, cal, thr)]
        for (rows, kept), z in zip(got, cal):
            w, n = int(z["mask_w"][q]), len(z["rows"])
            o = n * int(z["mask_w"][:q].sum())
            assert kept == w and "".join(rows).encode("latin-1") == z["mask_rows"][o:o + n * w].tobytes(), q
    assert any(0 < int(w) < z["rows"].shape[1] for z in cal for w in z["mask_w"])
