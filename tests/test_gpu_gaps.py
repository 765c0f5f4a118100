"""GPU: the gap structure and the ungapped rows of the summary stage (ka_sum_fam_gaps, ka_sum_fam_ungapped;
FamilySummary.gaps / ungapped / gap_stats; kalign_amd.summary.gap_stats / dealign) against the numpy restatement
(tests/sum_gap_restate.py) -- counts, row records, doubles and ungapped rows with np.array_equal / ==, no tolerance --,
against the gaps and cells the column table of the same handle gives (another kernel's exact integers) and against the
goldens recorded from the reference's compute_gap_stats (tests/golden/gap_*.npz, gapx_*.npz).

A wave walks one row in steps of 256 columns, four ballots of 64: widths stand at and around 64, 128 and 256.  The row
pass deals sixteen consecutive rows to a workgroup, a wave each, and adds up the rows of one family inside it before they
go to the family's sums; the ungap pass deals four: row counts stand at and around 4, 16 and 64, and the batches of small
families put several families, and the end of one, inside one workgroup."""
import numpy as np
import pytest

import sum_gap_restate as gr
from util import GOLDEN

pytestmark = pytest.mark.gpu

WIDTHS = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 259]
ROW_COUNTS = [1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65]
PROT = b"ACDEFGHIKLMNPQRSTVWY"
SHAPES = [(1, 1), (2, 5), (66, 9), (3, 300), (17, 64), (64, 17), (5, 257), (9, 130), (65, 70), (40, 3), (1, 40)]
ZERO = dict(gaps_ms=0.0, ungap_ms=0.0, gaps_launches=0, gaps_syncs=0, ungap_launches=0, ungap_syncs=0)


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


def same(x, y):
    """two gaps() dicts: integers and doubles equal (the doubles as bits), the row records too"""
    assert sorted(x) == sorted(y)
    for k in x:
        if k == "rows":
            assert x[k].dtype == np.int32 and x[k].shape == y[k].shape and np.array_equal(x[k], y[k]), np.argwhere(x[k] != y[k])[:5].tolist()
        elif isinstance(y[k], float):
            assert isinstance(x[k], float) and np.float64(x[k]).tobytes() == np.float64(y[k]).tobytes(), (k, x[k], y[k])
        else:
            assert type(x[k]) is int and x[k] == y[k], (k, x[k], y[k])
    return True


def check_batch(ctx, fams, gap=b"-"):
    """everything one handle says about the gaps of fams against the restatement and against its own column table;
    returns (gaps() with rows, ungapped rows) per family"""
    s = ctx.family_summary(fams, gap=gap)
    try:
        got, plain, summ = s.gaps(want_rows=True), s.gaps(), s.summary()
        rows, off = s.ungapped(want_offsets=True)
    finally:
        s.close()
    assert len(got) == len(plain) == len(rows) == len(fams)
    flat = []
    for f, fam in enumerate(fams):
        want = gr.gaps(fam, gap)
        assert same(got[f], want), f
        assert "rows" not in plain[f] and same(plain[f], {k: v for k, v in want.items() if k != "rows"}), f
        assert got[f]["total_gaps"] == summ[f]["gaps"] and got[f]["characters"] == summ[f]["cells"] - summ[f]["gaps"], f
        assert rows[f] == gr.ungapped(fam, gap)[0], f
        flat += rows[f]
    assert off.dtype == np.int64 and off.tolist() == np.concatenate([[0], np.cumsum([len(r) for r in flat])]).astype(np.int64).tolist()
    return list(zip(got, rows))


def test_widths_and_row_counts(ctx):
    rng = np.random.default_rng(21)
    check_batch(ctx, [family(rng, 5, w) for w in WIDTHS])
    check_batch(ctx, [family(rng, n, 70, b"ACGT", 0.4) for n in ROW_COUNTS])
    check_batch(ctx, [family(rng, n, w, gap_p=0.6) for n, w in ((3, 64), (4, 256), (5, 257), (64, 65))])


def put(w, fill, spans, other):
    a = bytearray(fill * w)
    for lo, hi in spans:
        a[lo:hi + 1] = other * (hi + 1 - lo)
    return bytes(a)


def test_blocks_placed_by_hand(ctx):
    """blocks that end at, start at and cross the edges of a ballot (column 63 | 64) and of a step (255 | 256), lone gaps
    and lone characters on either side of each; the block count of every row is a literal"""
    w = 700
    rows, blocks = [], []
    for e in (64, 256):                                          # e: the first column after the edge
        for spans, n in (([(e - 4, e - 1)], 1),                  # a block ends at the last column before the edge
                         ([(e - 3, e)], 1),                      # ... at the first after it (crossing)
                         ([(e - 1, e + 3)], 1),                  # starts at the last column before the edge
                         ([(e, e + 4)], 1),                      # ... at the first after it
                         ([(e - 1, e - 1)], 1),                  # a lone gap before the edge
                         ([(e, e)], 1),                          # ... after it
                         ([(e - 1, e)], 1),                      # one on each side: one block of two
                         ([(e - 2, e - 2), (e, e)], 2),          # two lone gaps with the last column before the edge between them
                         ([(e - 1, e - 1), (e + 1, e + 1)], 2),  # ... with the first column after it between them
                         ([(e - 9, e - 1), (e + 1, e + 9)], 2),  # a block that ends at the edge, the next one column later
                         ([(0, e - 1), (e + 1, w - 1)], 2)):     # everything but the first column after the edge
            rows.append(put(w, b"A", spans, b"-"))
            blocks.append(n)
        for spans, n in (([(e - 1, e - 1)], 2),                  # a lone character before the edge in a row of gaps
                         ([(e, e)], 2),                          # ... after it
                         ([(e - 1, e)], 2),
                         ([(e - 1, e - 1), (e + 1, e + 1)], 3)):
            rows.append(put(w, b"-", spans, b"A"))
            blocks.append(n)
    for spans, n in (([(10, 600)], 1),                           # a block across several steps
                     ([(63, 256)], 1), ([(64, 255)], 1), ([(0, 63), (128, 191), (256, 511)], 3), ([(0, 255), (512, 699)], 2),
                     ([(c, c) for c in range(1, w, 2)], 350), ([(c, c) for c in range(0, w, 2)], 350)):
        rows.append(put(w, b"A", spans, b"-"))
        blocks.append(n)
    assert len(rows) == 37
    got = check_batch(ctx, [rows, rows[::-1], rows[:1]])
    assert got[0][0]["rows"][:, 3].tolist() == blocks and got[1][0]["rows"][:, 3].tolist() == blocks[::-1]
    assert got[0][0]["n_gap_blocks"] == sum(blocks) == 756
    # leading and trailing of the rows of gaps with one character, by hand
    assert got[0][0]["rows"][11].tolist() == [1, 63, 636, 2] and got[0][0]["rows"][12].tolist() == [1, 64, 635, 2]
    assert got[0][0]["rows"][26].tolist() == [1, 255, 444, 2] and got[0][0]["rows"][27].tolist() == [1, 256, 443, 2]


def test_nothing_past_a_rows_end(ctx):
    """rows without a gap, and rows whose first and last column are gaps: a lane that took the byte after a row (0), the
    next row's first byte (a gap) or a byte past the upload for a column would change trailing or the blocks.  With the gap
    0x00 the byte after a row would itself be a gap.  The families stand last in the batch (the last row ends the upload)
    and first."""
    rng = np.random.default_rng(22)
    odd = [w for w in WIDTHS if w % 4]
    assert odd == [1, 2, 63, 65, 127, 129, 255, 257, 259]
    rand = [family(rng, 5, w) for w in (64, 256, 31)]
    for gap in (b"-", b"\x00"):
        full = [[bytes(rng.choice(np.frombuffer(PROT, np.uint8), size=w))] * 3 for w in odd]
        ends = [[put(w, b"A", [(0, 0), (w - 1, w - 1)], gap)] * 5 for w in odd]
        for fams, at in ((rand + full + ends, len(rand)), (ends[::-1] + full[::-1] + rand, 0)):
            got = check_batch(ctx, fams, gap)
            for k, w in enumerate(odd):
                f_full, f_ends = (at + k, at + len(odd) + k) if at else (2 * len(odd) - 1 - k, len(odd) - 1 - k)
                assert got[f_full][0]["rows"].tolist() == [[w, 0, 0, 0]] * 3, (w, at)
                want = [0, 1, 1, 1] if w == 1 else [0, 2, 2, 1] if w == 2 else [w - 2, 1, 1, 2]
                assert got[f_ends][0]["rows"].tolist() == [want] * 5, (w, at)


def test_row_forms(ctx):
    """all-gap rows (leading = trailing = width, one block), a row of one character at column 0 or at the last column, and a
    batch without a character: nothing to ungap, nothing launched for it"""
    fams = []
    for w in (1, 5, 64, 65, 256, 257):
        fams.append([b"-" * w, put(w, b"-", [(0, 0)], b"C"), put(w, b"-", [(w - 1, w - 1)], b"G"), b"-" * w])
    got = check_batch(ctx, fams)
    for f, w in enumerate((1, 5, 64, 65, 256, 257)):
        b = 0 if w == 1 else 1
        assert got[f][0]["rows"].tolist() == [[0, w, w, 1], [1, 0, w - 1, b], [1, w - 1, 0, b], [0, w, w, 1]], w
        assert got[f][0]["terminal_gaps"] == 4 * w + 2 * (w - 1) and got[f][0]["internal_gaps"] == 0
        assert got[f][1] == [b"", b"C", b"G", b""]
    empty = [[b"-" * 70] * 3, [b"-"], [b"-" * 257] * 5]
    s = ctx.family_summary(empty)
    try:
        assert s.ungapped() == [[b""] * 3, [b""], [b""] * 5]
        st = s.gap_stats()
        assert (st["gaps_launches"], st["gaps_syncs"], st["ungap_launches"], st["ungap_syncs"], st["ungap_ms"]) == (2, 1, 0, 0, 0.0)
        g = s.gaps()
        assert [d["expansion_factor"] for d in g] == [0.0] * 3 and [d["n_gap_blocks"] for d in g] == [3, 1, 5]
        assert [d["terminal_gaps"] for d in g] == [420, 2, 2570] and s.ungapped(want_offsets=True)[1].tolist() == [0] * 10
    finally:
        s.close()
    check_batch(ctx, empty)


def test_bytes(ctx):
    """0x00, 0x01, 0x80 and 0xFF are characters; with another gap byte '-' is one too"""
    rng = np.random.default_rng(23)
    odd_bytes = bytes([0x00, 0x01, 0x80, 0xFF, 0x2D, 0x2E])
    got = check_batch(ctx, [family(rng, 6, 131, odd_bytes[:4] + b"AC", 0.3), [b"\x00-\xff", b"-\x01-", b"\x80\x80-"]])
    assert got[1][1] == [b"\x00\xff", b"\x01", b"\x80\x80"]
    got = check_batch(ctx, [family(rng, 6, 65, b"ACGT-", 0.3, gap=b"."), family(rng, 3, 64, b"ACGT", 0.3, gap=b"."), [b"-.-", b"--.", b"..."]], gap=b".")
    assert got[2][0]["rows"].tolist() == [[2, 0, 0, 1], [2, 0, 1, 1], [0, 3, 3, 1]] and got[2][1] == [b"--", b"--", b""]
    got = check_batch(ctx, [family(rng, 4, 66, odd_bytes[:3] + b"-", 0.3, gap=b"\xff"), [b"-\xff-", b"\xff\xff-"]], gap=b"\xff")
    assert got[1][0]["rows"].tolist() == [[2, 0, 0, 1], [1, 2, 0, 1]] and got[1][1] == [b"--", b"-"]


def test_a_family_in_a_batch_equals_the_family_alone(ctx):
    rng = np.random.default_rng(24)
    fams = [family(rng, n, w, PROT if k % 2 else b"ACGTacgu", [0.0, 0.3, 0.7][k % 3]) for k, (n, w) in enumerate(SHAPES)]
    assert len(fams) == 11
    batch = check_batch(ctx, fams)
    for f, rows in enumerate(fams):
        alone = check_batch(ctx, [rows])                          # (a batch of one)
        assert same(alone[0][0], batch[f][0]) and alone[0][1] == batch[f][1], f


def test_goldens(ctx):
    """the reference's twelve fields through the fronts with its names: one alignment at a time, and all in one call"""
    from kalign_amd import summary
    cases = gr.goldens(GOLDEN)
    assert len(cases) >= 19 + 6
    alns = [[r.decode("latin-1") for r in rows] for _, rows, _ in cases]
    both = summary.gap_stats_families(ctx, alns)
    assert len(both) == len(cases)
    for (name, rows, want), aln, b in zip(cases, alns, both):
        one = summary.gap_stats(ctx, aln)
        assert same(one, b), name
        for k in gr.FIELDS:
            if k in gr.VALUES:
                assert np.float64(one[k]).tobytes() == want[k].tobytes(), (name, k, one[k], float(want[k]))
            else:
                assert one[k] == int(want[k]), (name, k, one[k], int(want[k]))
        assert same(summary.gap_stats(ctx, rows), one), name      # (bytes rows)


def test_dealign_round_trips(ctx):
    from kalign_amd import summary
    rng = np.random.default_rng(25)
    fams = [family(rng, n, w, gap_p=[0.0, 0.3, 0.9][k % 3]) for k, (n, w) in enumerate(SHAPES)]
    text = [[r.decode("latin-1") for r in f] if k % 2 else f for k, f in enumerate(fams)]
    got = summary.dealign_families(ctx, text)
    for k, (f, g) in enumerate(zip(fams, got)):
        want = [r.replace(b"-", b"") for r in f]
        assert g == ([r.decode("latin-1") for r in want] if k % 2 else want), k
    assert summary.dealign(ctx, ["AC-G-", "-----", "--T--"]) == ["ACG", "", "T"]
    assert summary.dealign(ctx, [b"AC-G-", b"-----"]) == [b"ACG", b""]
    s = ctx.family_summary(fams)
    try:
        rows, off = s.ungapped(want_offsets=True)
    finally:
        s.close()
    flat = [r for f in rows for r in f]
    assert off.tolist() == np.concatenate([[0], np.cumsum([len(r) for r in flat])]).tolist() and len(off) == sum(len(f) for f in fams) + 1


def test_fronts_refuse_as_the_module_does(ctx):
    from kalign_amd import KalignAmdError, summary
    for one, many in ((summary.gap_stats, summary.gap_stats_families), (summary.dealign, summary.dealign_families)):
        with pytest.raises(ValueError, match="Empty alignment provided"):
            one(ctx, [])
        with pytest.raises(ValueError, match="same length"):
            one(ctx, ["AC", "A"])
        with pytest.raises(ValueError, match="Empty list of alignments"):
            many(ctx, [])
        with pytest.raises(KalignAmdError, match="width 0"):
            many(ctx, [["AC"], ["", ""]])


def outputs(s):
    return (s.columns(), s.summary(), s.consensus(0.5, want_ambiguous=True), s.keep(0.5), s.compact(0.5), s.identity(want_counts=True))


def same_outputs(x, y):
    return (all(np.array_equal(p[k], q[k]) for p, q in zip(x[0], y[0]) for k in p) and x[1] == y[1] and x[2] == y[2] and
            all(np.array_equal(p, q) for p, q in zip(x[3], y[3])) and x[4] == y[4] and
            all(np.array_equal(a, b) for p, q in zip(x[5], y[5]) for a, b in zip(p, q)))


def test_handle(ctx):
    from kalign_amd import KalignAmdError
    rng = np.random.default_rng(26)
    fams = [family(rng, n, w) for n, w in SHAPES]
    seen = []
    for batch, ungap_first in ((fams[8:9], False), (fams, False), (fams, True)):
        s = ctx.family_summary(batch)
        try:
            assert s.gap_stats() == ZERO
            before, six, three = outputs(s), s.stats(), s.identity_stats()
            assert s.gap_stats() == ZERO
            if ungap_first:                                       # the ungapped rows first: the row pass runs for them
                rows = s.ungapped()
                first = s.gaps(want_rows=True)
            else:
                first = s.gaps(want_rows=True)
                mid = s.gap_stats()
                assert (mid["gaps_launches"], mid["gaps_syncs"], mid["ungap_launches"], mid["ungap_syncs"]) == (2, 1, 0, 0)
                assert mid["gaps_ms"] > 0.0 and mid["ungap_ms"] == 0.0
                rows = s.ungapped()
                assert {k: v for k, v in s.gap_stats().items() if k.startswith("gaps")} == {k: v for k, v in mid.items() if k.startswith("gaps")}
            st = s.gap_stats()
            assert (st["gaps_launches"], st["gaps_syncs"], st["ungap_launches"], st["ungap_syncs"]) == (2, 1, 1, 1)
            assert st["gaps_ms"] > 0.0 and st["ungap_ms"] > 0.0
            assert s.stats() == six and s.identity_stats() == three   # (the values of the other calls are theirs)
            # second calls copy what the first left: nothing is launched, the six values are as they were
            again = s.gaps(want_rows=True)
            assert all(same(x, y) for x, y in zip(first, again)) and s.ungapped() == rows and s.gap_stats() == st
            assert all(same(x, gr.gaps(f)) for x, f in zip(first, batch))
            # the handle's other outputs are what they were, and these after them too
            assert same_outputs(outputs(s), before) and s.identity_stats() == three
            assert s.ungapped() == rows and all(same(x, y) for x, y in zip(first, s.gaps(want_rows=True))) and s.gap_stats() == st
            seen.append(tuple(st[k] for k in ("gaps_launches", "gaps_syncs", "ungap_launches", "ungap_syncs")))
        finally:
            s.close()
        for call in (s.gaps, s.ungapped, s.gap_stats):
            with pytest.raises(KalignAmdError, match="the summary is closed"):
                call()
    assert seen[0] == seen[1] == seen[2]                          # one family, eleven families, either order


def test_a_small_cap_is_refused_with_nothing_launched(ctx):
    from kalign_amd import api
    fams = [[b"AC-G-", b"--T--"], [b"-", b"A"]]
    s = ctx.family_summary(fams)
    try:
        six = s.stats()
        assert s.L.ka_sum_fam_ungapped_size(s.h) == 5
        buf, off = np.zeros(8, np.uint8), np.full(5, -1, np.int64)
        assert s.L.ka_sum_fam_ungapped(s.h, api._ptr(buf), 4, api._ptr(off)) != 0
        assert s.L.ka_last_error().decode() == "ka_sum_fam_ungapped: 4 bytes do not hold the ungapped rows (5)"
        assert s.gap_stats() == ZERO and s.stats() == six and not buf.any() and (off == -1).all()
        assert s.L.ka_sum_fam_ungapped(s.h, None, 5, None) != 0 and s.L.ka_last_error().decode() == "ka_sum_fam_ungapped: bad arguments"
        assert s.gap_stats() == ZERO
        # the handle goes on as before; a cap of exactly the size is enough
        assert s.L.ka_sum_fam_ungapped(s.h, api._ptr(buf), 5, api._ptr(off)) == 0
        assert buf.tobytes() == b"ACGTA\0\0\0" and off.tolist() == [0, 3, 4, 4, 5]
        assert s.ungapped() == [[b"ACG", b"T"], [b"", b"A"]] and s.gaps()[0]["n_gap_blocks"] == 4
    finally:
        s.close()
