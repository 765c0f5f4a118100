"""A numpy restatement of the alignment comparison (lib/src/msa_cmp.c) for the tests: every counter of ka_cmp_score,
vectorised per sequence i, and the final doubles in the reference's expressions."""
import numpy as np


def is_res(a):
    return (np.asarray(a, np.uint8) | 32) - 97 < 26


def maps(rows):
    """(res[N][W] = residue index at column or -1, col[s] = columns of s's residues)"""
    a = np.frombuffer(b"".join(r.encode() if isinstance(r, str) else bytes(r) for r in rows), np.uint8).reshape(len(rows), -1)
    m = is_res(a)
    res = np.where(m, np.cumsum(m, axis=1) - 1, -1).astype(np.int64)
    col = [np.flatnonzero(m[s]) for s in range(len(rows))]
    return res, col, m


def scored_mask(rows, max_gap_frac=-1.0, column_mask=None):
    _, _, m = maps(rows)
    if column_mask is not None:
        return np.asarray(column_mask) != 0
    if np.float32(max_gap_frac) < 0:
        return np.ones(m.shape[1], bool)
    ngaps = (~m).sum(axis=0)
    return (ngaps.astype(np.float32) / np.float32(m.shape[0])) <= np.float32(max_gap_frac)


def counts(ref, test, scored):
    """the twelve counts of ka_cmp_score (include/kalign_amd.h order)"""
    resR, colR, mR = maps(ref)
    resT, colT, _ = maps(test)
    N = len(ref)
    ra = ta = ia = ig = rs = cs = 0
    for i in range(N):
        keep = np.arange(N) != i
        pR = resR[keep][:, colR[i]]
        pT = resT[keep][:, colT[i]]
        sc = scored[colR[i]][None, :]
        al = pR >= 0
        same = al & (pR == pT)
        ra += int(al.sum()); ta += int((pT >= 0).sum()); ia += int(same.sum()); ig += int(((pR < 0) & (pT < 0)).sum())
        rs += int((al & sc).sum()); cs += int((same & sc).sum())
    all_ = (N - 1) * sum(len(c) for c in colR)
    tc_total = tc_correct = 0
    # TC: the test column of every residue of a scored reference column with >= 2 residues
    tcol = [np.asarray(c) for c in colT]
    for c in np.flatnonzero(scored & (mR.sum(axis=0) >= 2)):
        rows = np.flatnonzero(mR[:, c])
        t = [tcol[s][resR[s, c]] for s in rows]
        tc_total += 1
        tc_correct += int(len(set(t)) == 1)
    return [ra, all_ - ra, ia, ig, ta, all_ - ta, rs, ta, cs, ia, tc_correct, tc_total]


def scores(c):
    """(sp float32, recall, precision, f1, tc) from the counts, in the reference's expressions"""
    a = float(np.uint64(c[2]) + np.uint64(c[3]))
    b = float(np.uint64(c[0]) + np.uint64(c[1]))
    sp = np.float32(100.0 * a / b)
    recall = c[8] / c[6] if c[6] > 0 else 0.0
    precision = c[9] / c[7] if c[7] > 0 else 0.0
    f1 = 2.0 * recall * precision / (recall + precision) if recall + precision > 0.0 else 0.0
    tc = c[10] / c[11] if c[11] > 0 else 0.0
    return sp, recall, precision, f1, tc
