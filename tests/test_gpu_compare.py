"""GPU: an alignment scored against a reference alignment (ka_cmp; kalign_amd.compare) against the reference's
kalign_msa_compare, kalign_msa_compare_detailed and kalign_msa_compare_with_mask (lib/src/msa_cmp.c) -- stored cases
(tests/golden/cmp_*.npz, make_golden_compare.py), live randomized cases when oracle/_ref is built, a numpy restatement
of every counter (cmp_restate.py), error paths and a property run at 4096 x ~400; and the job table behind score_many
(per-test tile geometry and LDS class, groups of 32) at its edges against the restatement.  Every value is compared
with ==."""
import glob
import os
import sys

import numpy as np
import pytest

from util import GOLDEN

pytestmark = pytest.mark.gpu

CASES = sorted(os.path.basename(f)[4:-4] for f in glob.glob(os.path.join(GOLDEN, "cmp_*.npz")))
sys.path.insert(0, GOLDEN)

import cmp_restate as R  # noqa: E402
from cmp_cases import check_restated, letters, placed  # noqa: E402


@pytest.fixture(scope="module")
def ctx():
    import kalign_amd
    c = kalign_amd.Context(0)
    yield c
    c.close()


def _gen():
    import make_golden_compare as G
    return G


def _ref():
    G = _gen()
    if not G.available():
        pytest.skip("oracle/_ref/libkalign_ref.so not built")
    return G


def _check(got, want_sp, poar, poar_i):
    assert np.float32(got["sp"]) == want_sp
    assert (got["recall"], got["precision"], got["f1"], got["tc"]) == tuple(float(x) for x in poar)
    assert (got["ref_pairs"], got["test_pairs"], got["common_pairs"]) == tuple(int(x) for x in poar_i)


def _check_ref_out(cmp, test, out, fracs, mask=None):
    for q, fr in enumerate(fracs):
        _check(cmp.score(test, max_gap_frac=float(fr)), out["sp"], out["poar"][q], out["poar_i"][q])
    if mask is not None:
        _check(cmp.score(test, column_mask=mask), out["sp"], out["mask_poar"], out["mask_i"])


@pytest.mark.parametrize("name", CASES)
def test_golden(ctx, name):
    from kalign_amd import compare as kc
    z = np.load(os.path.join(GOLDEN, "cmp_%s.npz" % name))
    names = [str(n) for n in z["names"]]
    ref = [str(r) for r in z["ref"]]
    tnames = [str(n) for n in z["test_names"]] if "test_names" in z.files else names
    for k, t in enumerate(z["tests"]):
        t = [str(r) for r in t]
        for q, fr in enumerate(z["fracs"]):
            got = kc.compare(ctx, list(zip(names, ref)), list(zip(tnames, t)), max_gap_frac=float(fr))
            _check(got, z["sp"][k], z["poar"][k, q], z["poar_i"][k, q])
        got = kc.compare(ctx, list(zip(names, ref)), list(zip(tnames, t)), column_mask=z["mask"])
        _check(got, z["sp"][k], z["mask_poar"][k], z["mask_i"][k])


def test_golden_boundary_and_all_gap_column(ctx):
    """1 gap in 5 rows at 0.2: (float)1 / (float)5 <= 0.2f scores the column; the all-gap column never counts for TC"""
    z = np.load(os.path.join(GOLDEN, "cmp_syn_gapfrac5.npz"))
    ref = [str(r) for r in z["ref"]]
    assert sum(r[10] == "-" for r in ref) == 1 and all(r[-1] == "-" for r in ref)
    assert R.scored_mask(ref, 0.2)[10] and not R.scored_mask(ref, 0.0)[10]
    test = [str(r) for r in z["tests"][0]]
    cmp = ctx.comparer(ref)
    for fr in (-1.0, 0.0, 0.19, 0.2, 0.5, 1.0):
        sc = R.scored_mask(ref, fr)
        assert cmp.score(test, max_gap_frac=fr)["tc_total"] == int((sc & (R.maps(ref)[2].sum(axis=0) >= 2)).sum())
    assert cmp.score(test, max_gap_frac=0.2)["ref_scored_pairs"] > cmp.score(test, max_gap_frac=0.19)["ref_scored_pairs"]
    # the all-gap column is scored at -1 but has no residue pair: TC leaves it out
    assert cmp.score(test)["tc_total"] == len(ref[0]) - 1 - int((R.maps(ref)[2].sum(axis=0) == 1).sum())
    cmp.close()


@pytest.mark.parametrize("seed,n,length,dna,extra", [(1, 2, 50, False, 0), (2, 7, 80, False, 5), (3, 33, 150, False, 0),
                                                       (4, 64, 120, True, 0), (5, 130, 60, False, 9)])
def test_live_random(ctx, seed, n, length, dna, extra):
    G = _ref()
    rng = np.random.RandomState(seed)
    ref, test = G.random_case(rng, n, length, dna=dna, width_extra=extra, noise=0.4)
    names = ["q%04d" % k for k in range(n)]
    mask = G.partial_mask(rng, len(ref[0]))
    out = G.reference_compare(names, ref, test, mask=mask)
    cmp = ctx.comparer(ref)
    _check_ref_out(cmp, test, out, G.FRACS, mask)
    cmp.close()


def test_dna_over_4096_residues(ctx):
    """the ensemble stage's 4096-residue limit does not apply here"""
    G = _ref()
    rng = np.random.RandomState(11)
    ref, test = G.random_case(rng, 6, 5200, dna=True, noise=0.2)
    assert max(sum(c != "-" for c in r) for r in ref) > 4096
    names = ["L%d" % k for k in range(6)]
    out = G.reference_compare(names, ref, test, fracs=np.array([-1.0, 0.5], np.float32))
    cmp = ctx.comparer(ref)
    _check_ref_out(cmp, test, out, [-1.0, 0.5])
    cmp.close()


def test_1024_against_reference(ctx):
    G = _ref()
    rng = np.random.RandomState(12)
    ref, test = G.random_case(rng, 1024, 400, noise=0.3)
    names = ["m%05d" % k for k in range(1024)]
    out = G.reference_compare(names, ref, test, fracs=np.array([0.2], np.float32))
    cmp = ctx.comparer(ref)
    _check_ref_out(cmp, test, out, [0.2])
    cmp.close()


def test_identical_alignments(ctx):
    G = _gen()
    ref, _ = G.random_case(np.random.RandomState(13), 40, 100)
    got = ctx.comparer(ref).score(ref)
    assert got["sp"] == 100.0 and got["recall"] == 1.0 and got["precision"] == 1.0 and got["tc"] == 1.0 and got["f1"] == 1.0


def test_lowercase_and_dots(ctx):
    G = _gen()
    ref, test = G.random_case(np.random.RandomState(14), 30, 90, noise=0.4)
    cmp = ctx.comparer(ref)
    a = cmp.score(test, max_gap_frac=0.5)
    b = cmp.score([r.lower().replace("-", ".") for r in test], max_gap_frac=0.5)
    c = ctx.comparer([r.lower().replace("-", ".") for r in ref]).score(test, max_gap_frac=0.5)
    assert a == b == c


def test_score_many_equals_single_calls(ctx):
    G = _gen()
    rng = np.random.RandomState(15)
    ref, _ = G.random_case(rng, 50, 300)
    tests = []                                            # 37: more than one device group of 32, widths differ
    for k in range(37):
        r = np.random.RandomState(200 + k)
        rows = []
        for row in ref:
            letters = "".join(c for c in row if c != "-")
            W = len(row) + (k % 3)
            cols = np.sort(r.choice(W, size=len(letters), replace=False))
            b = np.full(W, "-")
            b[cols] = list(letters)
            rows.append("".join(b))
        tests.append(rows)
    cmp = ctx.comparer(ref)
    many = cmp.score_many(tests, max_gap_frac=0.3)
    single = [cmp.score(t, max_gap_frac=0.3) for t in tests]
    assert many == single
    for t, got in zip(tests[:3], many):
        c = R.counts(ref, t, R.scored_mask(ref, 0.3))
        assert [got[k] for k in _keys()] == c


def _keys():
    from kalign_amd.api import CMP_COUNTS
    return CMP_COUNTS


def test_errors(ctx):
    from kalign_amd import KalignAmdError
    from kalign_amd import compare as kc
    ref = ["AC-D", "A-CD", "ACD-"]
    with pytest.raises(KalignAmdError):
        ctx.comparer(["AC-D"])                            # one sequence
    cmp = ctx.comparer(ref)
    with pytest.raises(KalignAmdError):
        cmp.score(["AC-D", "A-CD"])                       # row count
    with pytest.raises(KalignAmdError):
        cmp.score(["AC-D", "A-CD", "AC--"])               # residue count
    with pytest.raises(KalignAmdError):
        cmp.score(ref, column_mask=[1, 1, 1])             # mask length
    a = np.frombuffer("".join(ref).encode(), np.uint8)
    import ctypes as C
    assert ctx.L.ka_cmp_score(cmp.h, a.ctypes.data_as(C.c_void_p), 3, 4, None, None, None) != 0   # stride < alnlen
    assert cmp.score(ref)["sp"] == 100.0                 # still usable
    with pytest.raises(KalignAmdError):
        kc.compare(ctx, [("a", "AC-D"), ("a", "A-CD")], [("a", "AC-D"), ("b", "A-CD")])
    with pytest.raises(KalignAmdError):
        kc.compare(ctx, [("a", "AC-D"), ("b", "A-CD")], [("a", "AC-D"), ("c", "A-CD")])
    cmp.close()


def test_restatement_2048(ctx):
    G = _gen()
    ref, test = G.random_case(np.random.RandomState(16), 2048, 120, noise=0.4, width_extra=7)
    cmp = ctx.comparer(ref)
    for fr in (-1.0, 0.5):
        sc = R.scored_mask(ref, fr)
        want = R.counts(ref, test, sc)
        got = cmp.score(test, max_gap_frac=fr)
        assert [got[k] for k in _keys()] == want
        sp, rc, pr, f1, tc = R.scores(want)
        assert (np.float32(got["sp"]), got["recall"], got["precision"], got["f1"], got["tc"]) == (sp, rc, pr, f1, tc)
    cmp.close()


def test_property_4096(ctx):
    G = _gen()
    ref, test = G.random_case(np.random.RandomState(17), 4096, 400, noise=0.3)
    _, _, mR = R.maps(ref)
    _, _, mT = R.maps(test)
    nR, nT = mR.sum(axis=0).astype(np.int64), mT.sum(axis=0).astype(np.int64)
    N, sumL = len(ref), int(mR.sum())
    cmp = ctx.comparer(ref)
    got = cmp.score(test, max_gap_frac=0.5)
    sc = R.scored_mask(ref, 0.5)
    assert got["ref_total_aligned_pairs"] == int((nR * (nR - 1)).sum())
    assert got["test_pairs"] == got["test_total_aligned_pairs"] == int((nT * (nT - 1)).sum())
    assert got["ref_scored_pairs"] == int((nR * (nR - 1))[sc].sum())
    assert got["ref_total_gap_pairs"] == (N - 1) * sumL - got["ref_total_aligned_pairs"]
    assert got["test_total_gap_pairs"] == (N - 1) * sumL - got["test_total_aligned_pairs"]
    assert got["tc_total"] == int((sc & (nR >= 2)).sum())
    self_ = cmp.score(ref, max_gap_frac=0.5)
    assert self_["sp"] == 100.0 and self_["recall"] == 1.0 and self_["precision"] == 1.0 and self_["tc"] == 1.0
    assert self_["identical_aligned"] == self_["ref_total_aligned_pairs"]
    assert self_["identical_gaps"] == self_["ref_total_gap_pairs"]
    cmp.close()


# ---- the job table behind score_many: every test its own tile geometry and LDS class, groups of 32 ----
def _tests_of(rng, seqs, widths):
    return [placed(rng, seqs, W) for W in widths]


@pytest.mark.parametrize("WR", [7, 8, 9, 64, 65])
@pytest.mark.parametrize("N", [2, 16, 17, 32, 33, 47])
def test_score_many_tile_and_padding_edges(ctx, N, WR):
    """N at the KA_CMP_TI / KA_CMP_TJ boundaries, five tests narrower and wider than the reference and on both sides
    of the multiples of 8 (ka_cmp_pad); 17 x 64 with an all-gap reference column, 33 x 9 with a sequence without residues"""
    rng = np.random.RandomState(1000 * N + WR)
    free = 9 if (N, WR) == (17, 64) else None
    widths = [WR - 2, WR - 1, WR, WR + 1, (WR + 7) // 8 * 8 + 9]
    seqs = letters(rng, N, WR - 2, zero=(N, WR) == (33, 9))
    ref = placed(rng, seqs, WR, free)
    tests = _tests_of(rng, seqs, widths)
    assert free is None or all(r[free] == 45 for r in ref)
    mask = (rng.rand(WR) < 0.6).astype(np.int32)
    cmp = ctx.comparer(ref)
    for kw, scored in ((dict(), R.scored_mask(ref)), (dict(max_gap_frac=0.2), R.scored_mask(ref, 0.2)),
                       (dict(column_mask=mask), R.scored_mask(ref, -1.0, mask))):
        got = cmp.score_many(tests, **kw)
        assert len(got) == 5
        for g, t in zip(got, tests):
            check_restated(g, ref, t, scored)
    cmp.close()


def test_score_many_three_lds_classes_in_one_call(ctx):
    """3 x 600 against widths 610, 33000 and 5000: the walk stages 3, 1 and 3 row pairs -- up to 16 KiB, above 64 KiB
    and up to 64 KiB of LDS, one launch each, the widest test in the middle of the list"""
    rng = np.random.RandomState(71)
    seqs = letters(rng, 3, 600, alpha=b"ACGT")
    ref = placed(rng, seqs, 600)
    tests = _tests_of(rng, seqs, [610, 33000, 5000])
    assert 3 * (600 + 616) * 2 <= 16384 and (600 + 33000) * 2 > 65536 and 32768 < 3 * (600 + 5000) * 2 <= 65536
    cmp = ctx.comparer(ref)
    many = cmp.score_many(tests, max_gap_frac=0.5)
    assert many == [cmp.score(t, max_gap_frac=0.5) for t in tests]
    for g, t in zip(many, tests):
        check_restated(g, ref, t, R.scored_mask(ref, 0.5))
    cmp.close()


@pytest.fixture(scope="module")
def two_groups():
    """a 17 x 40 reference and 34 tests of differing widths: (ref, tests, the restated counts), left unchanged"""
    rng = np.random.RandomState(81)
    seqs = letters(rng, 17, 36)
    ref = placed(rng, seqs, 40)
    tests = _tests_of(rng, seqs, [36 + (5 * k) % 23 for k in range(34)])
    return ref, tests, [R.counts(ref, t, R.scored_mask(ref)) for t in tests]


def test_score_many_two_groups(ctx, two_groups):
    """33 tests: the job tables are rebuilt between the groups of 32 and every output lands at its k"""
    ref, tests, want = two_groups
    assert len({len(t[0]) for t in tests[:33]}) > 8
    cmp = ctx.comparer(ref)
    got = cmp.score_many(tests[:33])
    assert [[g[k] for k in _keys()] for g in got] == want[:33]
    for g, w in zip(got, want):
        sp, rc, pr, f1, tc = R.scores(w)
        assert (np.float32(g["sp"]), g["recall"], g["precision"], g["f1"], g["tc"]) == (sp, rc, pr, f1, tc)
    cmp.close()


def test_refused_test_in_the_second_group(ctx, two_groups):
    """a wrong letter count in test 32, a stride below the width of test 33: refused before anything runs (no output
    is written, not even the first group's), and the handle scores the valid tests afterwards"""
    import ctypes as C
    from kalign_amd import KalignAmdError
    from kalign_amd.api import _ptr
    ref, tests, want = two_groups
    cmp = ctx.comparer(ref)
    arrs = [np.frombuffer(b"".join(t), np.uint8) for t in tests]
    widths = np.array([len(t[0]) for t in tests], np.int32)

    def batch(arrs, strides):
        counts = np.full((34, 12), -1, np.int64)
        ptrs = (C.c_void_p * 34)(*[a.ctypes.data for a in arrs])
        rc = ctx.L.ka_cmp_score_batch(cmp.h, 34, ptrs, _ptr(np.asarray(strides, np.int64)), _ptr(widths), _ptr(counts), None, None)
        return rc, counts

    lost = tests[32][:3] + [b"-" * int(widths[32])] + tests[32][4:]       # row 3 lost its letters
    rc, counts = batch(arrs[:32] + [np.frombuffer(b"".join(lost), np.uint8)] + arrs[33:], widths)
    with pytest.raises(KalignAmdError, match=r"ka_cmp_score: test 32: row 3 holds 0 letters, its sequence \d+ \(every alignment"):
        ctx._chk(rc)
    assert (counts == -1).all()
    strides = widths.astype(np.int64)
    strides[33] -= 1
    rc, counts = batch(arrs, strides)
    with pytest.raises(KalignAmdError, match=r"ka_cmp_score: test 33: alignment width %d does not fit row stride %d" % (widths[33], widths[33] - 1)):
        ctx._chk(rc)
    assert (counts == -1).all()
    rc, counts = batch(arrs, widths)
    assert rc == 0 and counts.tolist() == want
    assert [[g[k] for k in _keys()] for g in cmp.score_many(tests[:33])] == want[:33]
    cmp.close()


def test_context_closes_comparers():
    import kalign_amd
    c = kalign_amd.Context(0)
    cmp = c.comparer(["AC-D", "A-CD"])
    c.close()
    assert cmp.h is None
