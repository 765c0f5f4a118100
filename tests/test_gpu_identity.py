"""GPU: the pairwise identity matrices of the summary stage (ka_sum_fam_identity, FamilySummary.identity,
kalign_amd.summary.pairwise_identity_matrix) against the numpy restatement (tests/sum_identity_restate.py) -- both count
matrices and the doubles with np.array_equal, no tolerance --, against the family sums the column table of the same handle
gives (another kernel's exact integers) and against the goldens recorded from python-kalign's kalign.utils
(tests/golden/idm_*.npz, ==).

Row counts stand at and around the tile of pairs (32 rows a side), widths at and around the word (4 columns), the 16-byte
read (16) and the staged chunk (128)."""
import glob
import os

import numpy as np
import pytest

import sum_identity_restate as ir
from util import GOLDEN

pytestmark = pytest.mark.gpu

ROW_COUNTS = [1, 2, 3, 31, 32, 33, 65]                   # 32: KA_SUM_IDM_T, the rows a side of a tile of pairs
WIDTHS = [1, 2, 3, 4, 5, 7, 8, 9, 127, 128, 129, 259]    # 128: KA_SUM_IDM_CHUNK, the columns staged per step
PROT = b"ACDEFGHIKLMNPQRSTVWY"


@pytest.fixture(scope="module")
def ctx():
    import kalign_amd
    c = kalign_amd.Context(0)
    yield c
    c.close()


def family(rng, n, w, alphabet=PROT, gap_p=0.3, gap=b"-"):
    a = rng.choice(np.frombuffer(alphabet, np.uint8), size=(n, w))
    a[rng.random((n, w)) < gap_p] = gap[0]
    return [r.tobytes() for r in a]


def check_batch(ctx, fams, gap=b"-"):
    """the three matrices of every family of one handle against the restatement, and their upper sums against the handle's
    own family sums; returns the device's (identity, matches, compared) per family"""
    s = ctx.family_summary(fams, gap=gap)
    try:
        got, summ = s.identity(want_counts=True), s.summary()
        plain = s.identity()
    finally:
        s.close()
    assert len(got) == len(plain) == len(fams)
    for f, rows in enumerate(fams):
        ident, m, c = got[f]
        wi, wm, wc = ir.identity(rows, gap)
        n = len(rows)
        assert ident.dtype == np.float64 and m.dtype == np.int32 and c.dtype == np.int32
        assert ident.shape == m.shape == c.shape == (n, n)
        assert np.array_equal(m, wm), (f, np.argwhere(m != wm)[:5].tolist())
        assert np.array_equal(c, wc), (f, np.argwhere(c != wc)[:5].tolist())
        assert np.array_equal(ident, wi), (f, np.argwhere(ident != wi)[:5].tolist())
        assert np.array_equal(plain[f], ident), f
        assert ir.upper_sums(m, c) == (summ[f]["matching_pairs"], summ[f]["compared_pairs"]), f
    return got


def test_row_counts_at_the_tile_edges(ctx):
    rng = np.random.default_rng(11)
    check_batch(ctx, [family(rng, n, 70, b"ACGT", 0.4) for n in ROW_COUNTS])


def test_widths_at_the_word_and_chunk_edges(ctx):
    """... and nothing past a row's end is counted: in a family of identical rows without gaps every count is the width, and
    the 0 byte after a row or the next row's first bytes would make it larger.  That family stands last in the batch (its
    last row ends the upload) and first."""
    rng = np.random.default_rng(12)
    rand = [family(rng, 5, w) for w in WIDTHS]
    same = [[bytes(rng.choice(np.frombuffer(PROT, np.uint8), size=w))] * 3 for w in WIDTHS if w % 4]
    assert len(same) == 9
    for fams, at in ((rand + same, len(rand)), (same[::-1] + rand, 0)):
        got = check_batch(ctx, fams)
        for k in range(len(same)):
            w = len(fams[at + k][0])
            ident, m, c = got[at + k]
            assert (m == w).all() and (c == w).all() and (ident == 1.0).all(), w


def test_a_family_in_a_batch_equals_the_family_alone(ctx):
    rng = np.random.default_rng(13)
    shapes = [(1, 1), (2, 5), (66, 9), (3, 300), (17, 64), (64, 17), (5, 257), (9, 130), (65, 70), (40, 3), (1, 40)]
    fams = [family(rng, n, w, PROT if k % 2 else b"ACGTacgu", [0.0, 0.3, 0.7][k % 3]) for k, (n, w) in enumerate(shapes)]
    assert len(fams) == 11
    batch = check_batch(ctx, fams)
    for f, rows in enumerate(fams):
        alone = check_batch(ctx, [rows])                          # (a batch of one)
        assert all(np.array_equal(x, y) for x, y in zip(alone[0], batch[f])), f


def lanes(cols):
    """columns [n, m] -> rows in which every column of cols stands once in each of the four byte lanes of a word: four
    copies, an 'A' column after each, m a multiple of 4"""
    cols = np.asarray(cols, np.uint8)
    n, m = cols.shape
    assert m % 4 == 0
    a = np.concatenate([np.concatenate([cols, np.full((n, 1), ord("A"), np.uint8)], axis=1)] * 4, axis=1)
    for j in range(m):
        assert sorted((r * (m + 1) + j) % 4 for r in range(4)) == [0, 1, 2, 3]
    return [r.tobytes() for r in a]


def test_bytes(ctx):
    """the zero-byte test of the packed compare at every byte value that a short form of it gets wrong"""
    rng = np.random.default_rng(14)
    # bytes that differ by exactly 0x01 ('A' / '@') on either side of a column that matches; 0x00 / 0x01 beside equal bytes
    one = [(0x41, 0x40), (0x47, 0x47), (0x40, 0x41), (0x47, 0x47), (0x47, 0x47), (0x41, 0x40), (0x00, 0x00), (0x01, 0x00),
           (0x00, 0x00), (0x00, 0x01), (0x00, 0x00), (0x47, 0x47)]
    # the high bit: 0x00 / 0x80, 0x7F / 0xFF differ; 0x80 / 0x80, 0xFF / 0xFF match
    high = [(0x00, 0x80), (0x7F, 0xFF), (0x80, 0x80), (0xFF, 0xFF), (0x80, 0x00), (0xFF, 0x7F), (0x80, 0x7F), (0x00, 0x00)]
    case = [(0x41, 0x61), (0x61, 0x61), (0x61, 0x41), (0x41, 0x41)]
    fams = []
    for pairs in (one, high, case, one + high + case):
        t = np.array(pairs, np.uint8).T
        third = t[0].copy()
        third[::3] = ord("-")
        fams.append(lanes(np.vstack([t, third[None, :]])))
    got = check_batch(ctx, fams)
    # rows 0 and 1 by hand, over the four copies and their 'A' columns: 7 of `one`'s 12 columns match, 3 of `high`'s 8, 2 of
    # `case`'s 4
    assert got[0][1][0, 1] == 4 * 7 + 4 and got[0][2][0, 1] == 4 * 12 + 4
    assert got[1][1][0, 1] == 4 * 3 + 4 and got[1][2][0, 1] == 4 * 8 + 4
    assert got[2][1][0, 1] == 4 * 2 + 4 and got[2][2][0, 1] == 4 * 4 + 4
    # the bytes 0x01, 0x80 and 0xFF inside rows, as tests/test_gpu_summary.py places them
    b = np.frombuffer(b"".join(family(rng, 5, 70, b"ACGU", 0.2)), np.uint8).reshape(5, 70).copy()
    b[1:3, 3] = 0x01
    b[[0, 4], 64] = 0x80
    b[2:5, 69] = 0xFF
    # upper and lower case of one letter in one column
    check_batch(ctx, [[r.tobytes() for r in b], [b"Aa", b"aA", b"AA", b"a-", b"Aa", b"aa"]])


def test_gaps(ctx):
    rng = np.random.default_rng(15)
    a = np.frombuffer(b"".join(family(rng, 7, 130)), np.uint8).reshape(7, 130).copy()
    a[3, :] = ord("-")
    got = check_batch(ctx, [[r.tobytes() for r in a], [b"AC--", b"--GT"], [b"-"], [b"----", b"----"]])
    ident, m, c = got[0]
    assert ident[3, 3] == 1.0 and m[3, 3] == 0 and c[3, 3] == 0
    other = np.arange(7) != 3
    assert (ident[3, other] == 0.0).all() and (ident[other, 3] == 0.0).all() and not m[3].any() and not c[3].any() and not c[:, 3].any()
    assert got[1][0].tolist() == [[1.0, 0.0], [0.0, 1.0]] and got[1][2].tolist() == [[2, 0], [0, 2]]
    assert got[2][0].tolist() == [[1.0]] and got[2][2].tolist() == [[0]]
    assert got[3][0].tolist() == [[1.0, 0.0], [0.0, 1.0]]
    # another gap byte: '-' is then a character like any other
    fams = [family(rng, 6, 65, b"ACGT-", 0.3, gap=b"."), family(rng, 3, 64, b"ACGT", 0.3, gap=b"."), [b"-.-", b"--."]]
    got = check_batch(ctx, fams, gap=b".")
    assert got[2][1].tolist() == [[2, 1], [1, 2]] and got[2][2].tolist() == [[2, 1], [1, 2]]
    check_batch(ctx, [family(rng, 4, 66, b"ACGT-", 0.3, gap=b"\xff"), [b"-\xff-", b"--\xff"]], gap=b"\xff")


CASES = sorted(os.path.basename(p)[4:-4] for p in glob.glob(os.path.join(GOLDEN, "idm_*.npz")))


def test_goldens(ctx):
    """the reference's matrices through the fronts with its names: one alignment at a time, and all in one call"""
    from kalign_amd import summary
    assert len(CASES) >= 15
    alns = [[r.tobytes().decode("latin-1") for r in np.load(os.path.join(GOLDEN, "sum_%s.npz" % c))["rows"]] for c in CASES]
    want = [np.load(os.path.join(GOLDEN, "idm_%s.npz" % c))["identity"] for c in CASES]
    for name, aln, w in zip(CASES, alns, want):
        got = summary.pairwise_identity_matrix(ctx, aln)
        assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == w.shape and (got == w).all(), name
    both = summary.pairwise_identity_matrices(ctx, alns)
    assert len(both) == len(want) and all(g.shape == w.shape and (g == w).all() for g, w in zip(both, want))


def test_fronts_refuse_as_the_module_does(ctx):
    from kalign_amd import KalignAmdError, summary
    with pytest.raises(ValueError, match="Empty alignment provided"):
        summary.pairwise_identity_matrix(ctx, [])
    with pytest.raises(ValueError, match="same length"):
        summary.pairwise_identity_matrix(ctx, ["AC", "A"])
    with pytest.raises(ValueError, match="Empty list of alignments"):
        summary.pairwise_identity_matrices(ctx, [])
    with pytest.raises(KalignAmdError, match="width 0"):
        summary.pairwise_identity_matrices(ctx, [["AC"], ["", ""]])


def outputs(s):
    return (s.columns(), s.summary(), s.consensus(0.5, want_ambiguous=True), s.keep(0.5), s.compact(0.5))


def same_outputs(x, y):
    return (all(np.array_equal(p[k], q[k]) for p, q in zip(x[0], y[0]) for k in p) and x[1] == y[1] and x[2] == y[2] and
            all(np.array_equal(p, q) for p, q in zip(x[3], y[3])) and x[4] == y[4])


def test_handle(ctx):
    from kalign_amd import KalignAmdError
    rng = np.random.default_rng(16)
    shapes = [(1, 1), (2, 5), (66, 9), (3, 300), (17, 64), (64, 17), (5, 257), (9, 130), (65, 70), (40, 3), (1, 40)]
    fams = [family(rng, n, w) for n, w in shapes]
    seen = []
    for batch in (fams[8:9], fams):
        s = ctx.family_summary(batch)
        try:
            assert s.identity_stats() == dict(identity_ms=0.0, launches=0, syncs=0)
            before, six = outputs(s), s.stats()
            first = s.identity(want_counts=True)
            st = s.identity_stats()
            assert st["launches"] == 1 and st["syncs"] == 1 and st["identity_ms"] > 0.0
            assert s.stats() == six                               # (the six values of the other calls are theirs)
            # a second call copies what the first left: nothing is launched, the three values are as they were
            again = s.identity(want_counts=True)
            assert s.identity_stats() == st
            assert all(np.array_equal(x, y) for p, q in zip(first, again) for x, y in zip(p, q))
            assert all(np.array_equal(x, p[0]) for x, p in zip(s.identity(), first))
            assert s.identity_stats() == st
            # the handle's other outputs are what they were, and the matrices after them too
            assert same_outputs(outputs(s), before)
            assert all(np.array_equal(x, p[0]) for x, p in zip(s.identity(), first)) and s.identity_stats() == st
            seen.append((st["launches"], st["syncs"]))
        finally:
            s.close()
        with pytest.raises(KalignAmdError, match="the summary is closed"):
            s.identity()
        with pytest.raises(KalignAmdError, match="the summary is closed"):
            s.identity_stats()
    assert seen[0] == seen[1]                                     # one family, eleven families


def test_a_refused_batch_launches_nothing(ctx):
    """46341 rows: the matrices would hold 2^31 entries and more.  Refused before anything is allocated or launched, and the
    handle goes on as before."""
    from kalign_amd import KalignAmdError
    s = ctx.family_summary([[b"A"] * 46341])
    try:
        six, summ = s.stats(), s.summary()
        with pytest.raises(KalignAmdError, match="ka_sum_fam_identity: family 0: 46341 rows bring the matrices to 2147488281 entries; "
                                                 "a batch holds fewer than 2\\^31"):
            s.identity()
        assert s.identity_stats() == dict(identity_ms=0.0, launches=0, syncs=0) and s.stats() == six
        assert s.summary() == summ and s.consensus(0.5) == [b"A"]
        assert summ[0]["matching_pairs"] == 46341 * 46340 // 2
    finally:
        s.close()
