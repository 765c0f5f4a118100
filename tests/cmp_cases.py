"""Random alignments for the comparison tests (test_gpu_compare.py, test_gpu_compare_families.py): the same letters
placed independently in alignments of chosen widths, and the check of a result against the numpy restatement."""
import sys

import numpy as np

from util import GOLDEN

sys.path.insert(0, GOLDEN)

import cmp_restate as R  # noqa: E402


def keys():
    from kalign_amd.api import CMP_COUNTS
    return CMP_COUNTS


def letters(rng, N, cap, zero=False, alpha=b"ACDEFGHIKLMNPQRSTVWY"):
    """N sequences (uint8 arrays) of cap // 2 .. cap letters; with `zero` sequence 1 has none"""
    lens = rng.randint(max(1, cap // 2), cap + 1, size=N)
    if zero:
        lens[1] = 0
    a = np.frombuffer(alpha, np.uint8)
    return [a[rng.randint(0, len(a), size=n)] for n in lens]


def placed(rng, letters, W, free=None):
    """one row per sequence: its letters (uint8 arrays) at random columns of W, never column `free`"""
    cols_ok = np.array([c for c in range(W) if c != free])
    rows = []
    for seq in letters:
        row = np.full(W, ord("-"), np.uint8)
        row[np.sort(rng.choice(cols_ok, size=len(seq), replace=False))] = seq
        rows.append(row.tobytes())
    return rows


def family(rng, N, WR, WT, free=None, zero=False, alpha=b"ACDEFGHIKLMNPQRSTVWY"):
    """(reference rows, test rows) of N sequences: the same letters placed independently in WR and in WT columns; with
    `free` that reference column stays all gaps, with `zero` sequence 1 has no residue"""
    seqs = letters(rng, N, min(WR - (free is not None), WT), zero, alpha)
    return placed(rng, seqs, WR, free), placed(rng, seqs, WT)


def check_restated(got, ref, test, scored):
    want = R.counts(ref, test, scored)
    assert [got[k] for k in keys()] == want
    sp, rc, pr, f1, tc = R.scores(want)
    assert (np.float32(got["sp"]), got["recall"], got["precision"], got["f1"], got["tc"]) == (sp, rc, pr, f1, tc)
