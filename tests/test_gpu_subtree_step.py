"""The wave-local subtree engine's paired DP step (ka_subtree.h, ka_sub_pass) at its edges, against the oracle bit for bit.

Deep Hirschberg windows of at most 64 rows run as subtrees; their passes take the steps two at a time.  The shapes here put
the windows' edges where the pairing and the lane constants matter: roots of 1, 2, 63 and 64 rows, windows of one to three
columns, windows on column 0 or on the last column (terminal gaps), and odd step counts (the extra step of a pair).  Every
kind of task (seq-seq, seq-profile, profile-profile), protein and nucleotide, with and without anchor consistency."""
import os

import numpy as np
import pytest

from util import GOLDEN

pytestmark = pytest.mark.gpu

# (row sequence length, column sequence length): the shorter side is the one the recursion splits down to its leaves
SHAPES = [(1, 1), (1, 3), (2, 2), (2, 3), (3, 64), (63, 1), (63, 2), (63, 3), (64, 1), (64, 3), (64, 64), (63, 65),
          (65, 63), (64, 129), (127, 40), (128, 64), (5, 200), (200, 7)]


def _codes(rng, la, lb, alpha, n):
    """n related sequences: the first la letters long, the rest around lb (edits, indels and ragged ends)"""
    base = rng.randint(0, alpha, max(la, lb) + 8).astype(np.uint8)
    out = [np.ascontiguousarray(base[:la])]
    for k in range(1, n):
        L = lb if k == 1 else max(1, lb + rng.randint(-2, 3))
        s = base[:L].copy()
        idx = rng.rand(L) < 0.3
        s[idx] = rng.randint(0, alpha, int(idx.sum()))
        if L > 4 and rng.rand() < 0.5:                  # a deletion inside
            p = rng.randint(1, L - 2)
            s = np.concatenate([s[:p], s[p + 2:]])
        out.append(np.ascontiguousarray(s))
    return out


def _tasks(n, shape):
    if n == 2:
        return np.array([(0, 1, 2)], np.int32)                                  # seq-seq
    if shape == "caterpillar":
        return np.array([(0, 1, 3), (3, 2, 4)], np.int32)                       # seq-seq, then seq-profile
    return np.array([(0, 1, 4), (2, 3, 5), (4, 5, 6)], np.int32)                # two seq-seq, then profile-profile


def _check(oracle, codes, tasks, dna, k, tag):
    import kalign_amd
    z = np.load(os.path.join(GOLDEN, "param_tables.npz"))
    subm = z["subm_1_0"] if dna else z["subm_0_3"]
    scal = (z["scal_1_0"] if dna else z["scal_0_3"]).copy()
    dist = np.linspace(0.2, 1.1, len(codes)).astype(np.float32)
    ctx = kalign_amd.Context(0)
    recs, paths, gaps = ctx.msa_tree(codes, tasks, subm, scal, dist, n_anchors=k, weight=2.0)
    ctx.close()
    if k:
        orecs, opaths, ogaps, _, _, _ = oracle.msa_tree_cons(codes, tasks, subm, scal, dist, k, 2.0)
    else:
        orecs, opaths, ogaps, _ = oracle.msa_tree(codes, tasks, subm, scal, dist)
    for t, (r, o) in enumerate(zip(recs, orecs)):
        assert (r.plen, r.kind, r.swapped, r.meet, r.transition) == (o.plen, o.kind, o.swapped, o.meet, o.transition), (tag, t)
        assert r.score == o.score, (tag, t, r.score, o.score)
        assert np.array_equal(paths[r.path_off:r.path_off + r.plen + 2], opaths[o.path_off:o.path_off + o.plen + 2]), (tag, t)
    for a, b in zip(gaps, ogaps):
        assert np.array_equal(a, b), tag


@pytest.mark.parametrize("la,lb", SHAPES)
@pytest.mark.parametrize("dna", [False, True])
def test_seq_seq_edges(oracle, la, lb, dna):
    rng = np.random.RandomState(7 * la + lb + (1000 if dna else 0))
    codes = _codes(rng, la, lb, 4 if dna else 20, 2)
    _check(oracle, codes, _tasks(2, None), dna, 0, ("ss", la, lb, dna))


@pytest.mark.parametrize("la,lb", SHAPES)
@pytest.mark.parametrize("k", [0, 3])
def test_seq_profile_edges(oracle, la, lb, k):
    rng = np.random.RandomState(11 * la + lb + 31 * k)
    codes = _codes(rng, la, lb, 20, 3)
    _check(oracle, codes, _tasks(3, "caterpillar"), False, k, ("sp", la, lb, k))


@pytest.mark.parametrize("la,lb", SHAPES)
@pytest.mark.parametrize("k", [0, 3])
@pytest.mark.parametrize("dna", [False, True])
def test_profile_profile_edges(oracle, la, lb, k, dna):
    rng = np.random.RandomState(13 * la + lb + 37 * k + (2000 if dna else 0))
    codes = _codes(rng, la, lb, 4 if dna else 20, 4)
    _check(oracle, codes, _tasks(4, "balanced"), dna, k, ("pp", la, lb, k, dna))
