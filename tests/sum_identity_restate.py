"""A numpy statement of what the identity pass of the summary stage (ka_sum_fam_identity) returns for one family, written
from the stage's contract: a byte is a gap when it equals the gap byte, every other byte is a character and is compared as
a byte; compared[i][j] counts the columns where both rows hold a character, matches[i][j] those of them where the bytes
are equal (on the diagonal both are the characters of row i); identity is matches / compared off the diagonal, 0.0 where
nothing is compared, and 1.0 on the diagonal always.  The GPU tests hold the device to it, the host tests hold it to the
goldens recorded from python-kalign's kalign.utils.pairwise_identity_matrix (tests/golden/make_golden_identity.py)."""
import numpy as np

from sum_restate import to_array


def counts(rows, gap=b"-"):
    """(matches, compared): int32 [n, n], symmetric"""
    a = to_array(rows)
    n = a.shape[0]
    ch = a != gap[0]
    matches, compared = np.zeros((n, n), np.int32), np.zeros((n, n), np.int32)
    for i in range(n):
        both = ch[i][None, :] & ch
        compared[i] = both.sum(axis=1)
        matches[i] = (both & (a == a[i][None, :])).sum(axis=1)
    return matches, compared


def identity(rows, gap=b"-"):
    """(identity float64 [n, n], matches, compared)"""
    m, c = counts(rows, gap)
    ident = np.zeros(m.shape, np.float64)
    np.divide(m.astype(np.float64), c.astype(np.float64), out=ident, where=c > 0)      # one IEEE division per entry
    np.fill_diagonal(ident, 1.0)
    return ident, m, c


def upper_sums(m, c):
    """the sums over i < j of the two count matrices: a family's matching_pairs and compared_pairs"""
    iu = np.triu_indices(m.shape[0], 1)
    return int(m[iu].astype(np.int64).sum()), int(c[iu].astype(np.int64).sum())
