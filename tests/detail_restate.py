"""A numpy restatement of every output of ka_cmp_detail / ka_cmp_fam_detail (include/kalign_amd.h) for the tests: the three
counts of every residue, vectorised per sequence as cmp_restate.counts walks them, and the records of the test columns and
of the reference columns.  A column's flag comes from the set of columns its residues have in the other alignment (the
rule of _column_correctness), not from the counts: the tests hold the two against each other."""
import numpy as np

import cmp_restate as R


def _columns(res_own, col_other, offs, plane2):
    """the records of the columns of one alignment: res_own [N][W] its res map, col_other[s] the columns of s's residues in
    the other alignment, offs[s] the first flat residue of s"""
    N, W = res_own.shape
    k = np.zeros(W, np.int32)
    common = np.zeros(W, np.int64)
    correct = np.zeros(W, np.uint8)
    for c in range(W):
        rows = np.flatnonzero(res_own[:, c] >= 0)
        there = set(int(col_other[s][res_own[s, c]]) for s in rows)
        k[c] = len(rows)
        common[c] = sum(int(plane2[offs[s] + res_own[s, c]]) for s in rows)
        correct[c] = 1 if len(rows) <= 1 or len(there) == 1 else 0
    return dict(residues=k, common=common, correct=correct)


def detail(ref, test):
    """dict(res=[T, 3] int32, test_columns, ref_columns = dicts of residues, common, correct) of one family"""
    resR, colR, _ = R.maps(ref)
    resT, colT, _ = R.maps(test)
    N = len(ref)
    offs = np.concatenate([[0], np.cumsum([len(c) for c in colR])]).astype(np.int64)
    assert [len(c) for c in colR] == [len(c) for c in colT], "the two alignments hold the same sequences"
    res = np.zeros((int(offs[-1]), 3), np.int32)
    for i in range(N):
        keep = np.arange(N) != i
        pR = resR[keep][:, colR[i]]
        pT = resT[keep][:, colT[i]]
        res[offs[i]:offs[i + 1], 0] = (pR >= 0).sum(axis=0)
        res[offs[i]:offs[i + 1], 1] = (pT >= 0).sum(axis=0)
        res[offs[i]:offs[i + 1], 2] = ((pR >= 0) & (pR == pT)).sum(axis=0)
    return dict(res=res, test_columns=_columns(resT, colR, offs, res[:, 2]), ref_columns=_columns(resR, colT, offs, res[:, 2]))


def column_flags(ref, test):
    """the test columns' flags alone, vectorised over the columns: what a host without the device would run (the timing
    baseline of tools/compare_detail_time.py)"""
    _, colR, _ = R.maps(ref)
    resT, _, mT = R.maps(test)
    there = np.full(resT.shape, -1, np.int64)                    # the reference column of the residue at (s, c)
    for s in range(len(ref)):
        there[s, mT[s]] = colR[s]
    lo = np.where(mT, there, np.iinfo(np.int64).max).min(axis=0)
    hi = there.max(axis=0)
    return ((mT.sum(axis=0) <= 1) | (lo == hi)).astype(np.uint8)


def same(got, want):
    """every array of a detail result equal, dtype and shape included"""
    pairs = [(got["res"], want["res"])] + [(got[side][k], want[side][k]) for side in ("test_columns", "ref_columns")
                                           for k in ("residues", "common", "correct")]
    return all(a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b) for a, b in pairs)
