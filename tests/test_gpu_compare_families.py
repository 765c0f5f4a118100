"""GPU: a batch of families, each scored against its own reference alignment in one pass (ka_cmp_fam,
Context.family_comparer, kalign_amd.compare.compare_families) -- against the stored results of the real reference
(tests/golden/cmp_*.npz as one batch), the numpy restatement of every counter (cmp_restate.py) at the edges of the tile
geometry, the one-family Comparer, and the live reference when oracle/_ref is built.  Every value is compared with ==."""
import glob
import os
import sys

import numpy as np
import pytest

from util import GOLDEN

pytestmark = pytest.mark.gpu

sys.path.insert(0, GOLDEN)

import cmp_restate as R  # noqa: E402
from cmp_cases import check_restated, family, keys as _keys  # noqa: E402

FRACS = [float(np.float32(x)) for x in (-1.0, 0.0, 0.2, 0.5, 1.0)]    # as stored: float32


@pytest.fixture(scope="module")
def ctx():
    import kalign_amd
    c = kalign_amd.Context(0)
    yield c
    c.close()


# ---- 1. the stored results of the real reference, all cases as one batch ----
def test_golden_cases_as_one_batch(ctx):
    from kalign_amd import compare as kc
    refs, tests, want, masks = [], [], [], []
    files = sorted(glob.glob(os.path.join(GOLDEN, "cmp_*.npz")))
    assert len(files) == 21
    for path in files:
        z = np.load(path)
        names = [str(n) for n in z["names"]]
        tnames = [str(n) for n in z["test_names"]] if "test_names" in z.files else names
        assert [float(x) for x in z["fracs"]] == FRACS
        for k, t in enumerate(z["tests"]):
            r, tt = kc.pair_rows(list(zip(names, (str(x) for x in z["ref"]))), list(zip(tnames, (str(x) for x in t))))
            refs.append(r)
            tests.append(tt)
            masks.append(z["mask"])
            want.append(dict(sp=z["sp"][k], poar=z["poar"][k], poar_i=z["poar_i"][k], mask_poar=z["mask_poar"][k], mask_i=z["mask_i"][k]))
    assert len(refs) == 28 and min(len(r) for r in refs) == 2 and max(len(r) for r in refs) == 44
    assert min(len(r[0]) for r in refs) == 58 and max(len(r[0]) for r in refs) == 1753

    def check(got, w, q):
        poar, poar_i = (w["mask_poar"], w["mask_i"]) if q is None else (w["poar"][q], w["poar_i"][q])
        assert np.float32(got["sp"]) == w["sp"]
        assert (got["recall"], got["precision"], got["f1"], got["tc"]) == tuple(float(x) for x in poar)
        assert (got["ref_pairs"], got["test_pairs"], got["common_pairs"]) == tuple(int(x) for x in poar_i)

    cmp = ctx.family_comparer(refs)
    for q, fr in enumerate(FRACS):
        got = cmp.score(tests, max_gap_frac=fr)
        assert len(got) == 28
        for g, w in zip(got, want):
            check(g, w, q)
    for g, w in zip(cmp.score(tests, column_masks=masks), want):
        check(g, w, None)
    # every family its own rule: the fractions in turn, every third family its mask
    rule = [None if f % 3 == 2 else f % 5 for f in range(28)]
    got = cmp.score(tests, max_gap_frac=[FRACS[f % 5] for f in range(28)], column_masks=[masks[f] if rule[f] is None else None for f in range(28)])
    for g, w, q in zip(got, want, rule):
        check(g, w, q)
    st = cmp.stats()
    assert st["ref_maps_ms"] > 0 and st["walk_ms"] > 0
    cmp.close()


# ---- 2. the edges of the tile geometry ----
EDGE_N = [2, 3, 16, 17, 32, 33, 47]
EDGE_W = [1, 7, 8, 9, 15, 16, 17, 63, 64, 65]


@pytest.fixture(scope="module")
def edges():
    """families at the KA_CMP_TI / KA_CMP_TJ boundaries with widths at the ka_cmp_pad boundaries (test wider and narrower
    than its reference), one with an all-gap reference column, one with a sequence without residues, and 40 x ~600
    (WRp + WTp > 1024: TJ = 26 < 32, two j-tiles under the 64 KiB budget).  (refs, tests), left unchanged."""
    rng = np.random.RandomState(2026)
    refs, tests = [], []
    for k, N in enumerate(EDGE_N):
        for j in range(3):
            WR, WT = EDGE_W[(3 * k + j) % 10], EDGE_W[(7 * k + 3 * j + 4) % 10]
            r, t = family(rng, N, WR, WT)
            refs.append(r)
            tests.append(t)
    for WR, WT in ((1, 65), (65, 1), (1, 1)):
        r, t = family(rng, 3, WR, WT)
        refs.append(r)
        tests.append(t)
    r, t = family(rng, 17, 64, 63, free=9)
    assert all(x[9] == 45 for x in r)
    refs.append(r); tests.append(t)
    r, t = family(rng, 5, 17, 15, zero=True)
    assert set(r[1]) == {45} == set(t[1])
    refs.append(r); tests.append(t)
    r, t = family(rng, 40, 600, 610)
    refs.append(r); tests.append(t)
    widths = {(len(a[0]), len(b[0])) for a, b in zip(refs, tests)}
    assert {w for w, _ in widths} == set(EDGE_W) | {600} and any(a < b for a, b in widths) and any(a > b for a, b in widths)
    return refs, tests


@pytest.fixture(scope="module")
def edge_want(edges):
    """cmp_restate's twelve counts of every edge family with every column scored, computed once"""
    return [R.counts(r, t, R.scored_mask(r)) for r, t in zip(*edges)]


def test_tile_edges_against_the_restatement(ctx, edges, edge_want):
    refs, tests = edges
    cmp = ctx.family_comparer(refs)
    got = cmp.score(tests)
    for g, w in zip(got, edge_want):
        assert [g[k] for k in _keys()] == w
        sp, rc, pr, f1, tc = R.scores(w)
        assert (np.float32(g["sp"]), g["recall"], g["precision"], g["f1"], g["tc"]) == (sp, rc, pr, f1, tc)
    # the float rule with every family's own N, and a mask on every second family
    got = cmp.score(tests, max_gap_frac=0.2)
    for g, r, t in zip(got, refs, tests):
        check_restated(g, r, t, R.scored_mask(r, 0.2))
    rng = np.random.RandomState(5)
    masks = [(rng.rand(len(r[0])) < 0.6).astype(np.int32) if f % 2 else None for f, r in enumerate(refs)]
    got = cmp.score(tests, max_gap_frac=0.5, column_masks=masks)
    for g, r, t, m in zip(got, refs, tests, masks):
        check_restated(g, r, t, R.scored_mask(r, 0.5, m))
    cmp.close()


# ---- 3. a row pair above 64 KiB ----
def test_large_lds_family_beside_small_ones(ctx):
    rng = np.random.RandomState(31)
    big = family(rng, 3, 17000, 17003, alpha=b"ACGT")
    assert (17000 + 17008) * 2 > 65536
    small = [family(rng, 4, 30, 33), family(rng, 18, 70, 64)]
    refs, tests = zip(*[small[0], big, small[1]])
    got = ctx.family_comparer(refs).score(tests, max_gap_frac=0.4)
    for g, r, t in zip(got, refs, tests):
        assert g == ctx.comparer(r).score(t, max_gap_frac=0.4)
    assert got[1]["ref_total_aligned_pairs"] > 0


# ---- 4. more families than any grid cap ----
def test_2100_families(ctx):
    rng = np.random.RandomState(41)
    refs, tests = [], []
    for f in range(2100):
        r, t = family(rng, 2 + f % 2, rng.randint(5, 13), rng.randint(5, 13))
        refs.append(r)
        tests.append(t)
    got = ctx.family_comparer(refs).score(tests, max_gap_frac=0.0)
    assert len(got) == 2100
    for g, r, t in zip(got, refs, tests):
        assert [g[k] for k in _keys()] == R.counts(r, t, R.scored_mask(r, 0.0))


# ---- 5. independence ----
def test_families_do_not_see_each_other(ctx, edges, edge_want):
    refs, tests = edges
    F = len(refs)
    perm = np.random.RandomState(51).permutation(F)
    cmp = ctx.family_comparer([refs[p] for p in perm])
    first = cmp.score([tests[p] for p in perm])
    assert [[g[k] for k in _keys()] for g in first] == [edge_want[p] for p in perm]
    # other tests on the same handle (every reference against itself), then the first again
    self_ = cmp.score([refs[p] for p in perm])
    for g in self_:
        assert g["identical_aligned"] == g["ref_total_aligned_pairs"] and g["identical_gaps"] == g["ref_total_gap_pairs"]
        assert g["sp"] == 100.0 and g["tc_correct"] == g["tc_total"]
    assert cmp.score([tests[p] for p in perm]) == first
    cmp.close()


# ---- 6. equal to the loop of one-family comparers ----
def test_equal_to_the_loop(ctx):
    import make_golden_compare as G
    rng = np.random.RandomState(61)
    fams = [G.random_case(rng, 16, 120, noise=0.4, width_extra=k) for k in range(5)] + [G.random_case(rng, 64, 150, noise=0.3) for _ in range(3)]
    refs, tests = zip(*fams)
    masks = [G.partial_mask(rng, len(r[0])) for r in refs]
    cmp = ctx.family_comparer(refs)
    singles = [ctx.comparer(r) for r in refs]
    for kw, kw1 in ((dict(max_gap_frac=-1.0), None), (dict(max_gap_frac=0.2), None), (dict(column_masks=masks), masks)):
        got = cmp.score(tests, **kw)
        for f, (c, t) in enumerate(zip(singles, tests)):
            want = c.score(t, column_mask=masks[f]) if kw1 is not None else c.score(t, **kw)
            assert got[f] == want
    for c in singles:
        c.close()
    cmp.close()


# ---- 7. from alignment to scores ----
def test_run_families_rows_go_straight_in(ctx):
    import make_golden_compare as G
    from kalign_amd import compare as kc
    from kalign_amd import guide, synth
    from util import Golden
    g = Golden("tree_prot32x200")
    seqs = [synth.family(n, length, seed=700 + k) for k, (n, length) in enumerate([(3, 40), (8, 60), (17, 50), (33, 45)])]
    rows = ctx.run_families([(guide.encode_tree(s), guide.encode(s), s) for s in seqs], g.subm, g.scal, n_threads=2)
    refs = [G.left_packed([r.decode() for r in fam], extra=2) for fam in rows]
    cmp = ctx.family_comparer(refs)
    got = cmp.score(rows, max_gap_frac=0.2)
    cmp.close()
    assert got == [kc.compare(ctx, r, t, max_gap_frac=0.2) for r, t in zip(refs, rows)]
    assert got == kc.compare_families(ctx, refs, rows, max_gap_frac=0.2)


# ---- 8. errors: refused on the host, nothing launched ----
def test_refused_batches_leave_the_handle_usable(ctx, edges, edge_want):
    from kalign_amd import KalignAmdError
    refs, tests = edges
    refs, tests, want = refs[:6], tests[:6], edge_want[:6]
    with pytest.raises(KalignAmdError, match="ka_cmp_fam_create: family 1: 1 sequences; a comparison needs two at least"):
        ctx.family_comparer([refs[0], refs[1][:1]])
    with pytest.raises(KalignAmdError, match="ka_cmp_fam_create: empty family"):
        ctx.family_comparer([refs[0], []])
    wide = [b"AC" + b"-" * 40998, b"A" + b"-" * 40998 + b"C"]
    with pytest.raises(KalignAmdError, match=r"ka_cmp_fam_create: family 1: reference width 41000 exceeds the LDS of one CU"):
        ctx.family_comparer([refs[0], wide])
    cmp = ctx.family_comparer(refs + [[r[:30000] for r in wide]])
    ok = tests + [[r[:30000] for r in wide]]
    bad = list(ok)
    bad[3] = [bad[3][0]] + [b"-" * len(bad[3][0])] + bad[3][2:]   # a row that lost its letters
    with pytest.raises(KalignAmdError, match=r"ka_cmp_fam_score: family 3: row 1 holds 0 letters, its sequence \d+ \(every alignment"):
        cmp.score(bad)
    with pytest.raises(KalignAmdError, match="family 2: the test alignment has 1 rows, the reference 2"):
        cmp.score(ok[:2] + [ok[2][:1]] + ok[3:])
    with pytest.raises(KalignAmdError, match="family 0: mask length 3 != reference alignment length"):
        cmp.score(ok, column_masks=[[1, 1, 1]] + [None] * 6)
    with pytest.raises(KalignAmdError, match=r"ka_cmp_fam_score: family 6: reference width 30000 and test width 60000 together exceed the LDS"):
        cmp.score(tests + [[b"AC" + b"-" * 59998, b"A" + b"-" * 59999]])
    got = cmp.score(ok)
    assert [[g[k] for k in _keys()] for g in got[:6]] == want
    assert got[6]["sp"] == 100.0
    cmp.close()


def test_context_closes_family_comparers():
    import kalign_amd
    c = kalign_amd.Context(0)
    cmp = c.family_comparer([["AC-D", "A-CD"], ["GT", "GT", "G-"]])
    assert cmp.score([["ACD-", "A-CD"], ["GT", "GT", "-G"]])[1]["ref_total_aligned_pairs"] == 8
    c.close()
    assert cmp.h is None


# ---- 9. the live reference ----
def test_live_reference(ctx):
    import make_golden_compare as G
    if not G.available():
        pytest.skip("oracle/_ref/libkalign_ref.so not built")
    rng = np.random.RandomState(91)
    fams = [G.random_case(rng, 7, 80, width_extra=5, noise=0.4), G.random_case(rng, 33, 150, noise=0.4), G.random_case(rng, 20, 60, dna=True, noise=0.3)]
    refs, tests = zip(*fams)
    masks = [G.partial_mask(rng, len(r[0])) for r in refs]
    outs = [G.reference_compare(["q%04d" % k for k in range(len(r))], r, t, mask=m) for r, t, m in zip(refs, tests, masks)]
    cmp = ctx.family_comparer(refs)

    def check(got, out, q):
        poar, poar_i = (out["mask_poar"], out["mask_i"]) if q is None else (out["poar"][q], out["poar_i"][q])
        assert np.float32(got["sp"]) == out["sp"]
        assert (got["recall"], got["precision"], got["f1"], got["tc"]) == tuple(float(x) for x in poar)
        assert (got["ref_pairs"], got["test_pairs"], got["common_pairs"]) == tuple(int(x) for x in poar_i)

    for q, fr in enumerate(G.FRACS):
        for g, o in zip(cmp.score(tests, max_gap_frac=float(fr)), outs):
            check(g, o, q)
    for g, o in zip(cmp.score(tests, column_masks=masks), outs):
        check(g, o, None)
    cmp.close()
