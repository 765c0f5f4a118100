"""GPU: the summary stage over a batch of families (ka_sum_fam, Context.family_summary) against the numpy restatement
(tests/sum_restate.py) and the goldens recorded from python-kalign's kalign.utils (tests/golden/sum_*.npz): exact
integers, doubles compared with ==, strings byte for byte.

Widths stand at and around the column tile (64) and the row-gather chunk and scan block (256); row counts around the
eight waves that deal a tile's rows among them and the 64 lanes of a wave."""
import glob
import os

import numpy as np
import pytest

import sum_restate as sr
from util import GOLDEN

pytestmark = pytest.mark.gpu

WIDTHS = [1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1030]
ROW_COUNTS = [1, 2, 3, 4, 5, 63, 64, 65, 257]
CONS_THR = [0.0, 0.34, 0.5, 2.0 / 3.0, 1.0]
GAP_THR = [0.0, 0.25, 1.0 / 3.0, 0.5, 1.0]
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


def check_batch(ctx, fams, gap=b"-", cons_thr=(0.5,), gap_thr=(1.0, 0.5)):
    """every output of one handle over fams against the restatement of every family"""
    s = ctx.family_summary(fams, gap=gap)
    try:
        cols, summ = s.columns(), s.summary()
        for f, rows in enumerate(fams):
            want = sr.columns(rows, gap)
            for k in ("n_gap", "n_distinct", "top_char", "top_count", "same_pairs"):
                assert np.array_equal(cols[f][k], want[k]), (f, k, np.flatnonzero(cols[f][k] != want[k])[:5])
            assert summ[f] == sr.summary(rows, gap), f
        for t in cons_thr:
            got, amb = s.consensus(t, want_ambiguous=True)
            for f, rows in enumerate(fams):
                assert got[f] == sr.consensus(rows, t, gap), (f, t)
                assert amb[f] == sr.ambiguous(rows, gap), f
        for t in gap_thr:
            kp, out = s.keep(t), s.compact(t)
            for f, rows in enumerate(fams):
                assert kp[f].dtype == np.int32 and np.array_equal(kp[f], sr.keep(rows, t, gap=gap)), (f, t)
                assert out[f] == sr.compact(rows, t, gap=gap), (f, t)
    finally:
        s.close()


def test_widths_at_the_tile_and_chunk_edges(ctx):
    rng = np.random.default_rng(1)
    check_batch(ctx, [family(rng, 5 + k % 3, w) for k, w in enumerate(WIDTHS)], cons_thr=CONS_THR, gap_thr=GAP_THR)


def test_row_counts_at_the_wave_edges(ctx):
    rng = np.random.default_rng(2)
    check_batch(ctx, [family(rng, n, 70, b"ACGT", 0.4) for n in ROW_COUNTS], cons_thr=CONS_THR, gap_thr=GAP_THR)


def test_one_alignment_is_a_batch_of_one(ctx):
    rng = np.random.default_rng(3)
    check_batch(ctx, [family(rng, 9, 131)], cons_thr=CONS_THR, gap_thr=GAP_THR)
    check_batch(ctx, [[b"A"]])
    check_batch(ctx, [[b"-"]])


def test_contents(ctx):
    rng = np.random.default_rng(4)
    # an all-gap column (first, at a tile edge and last) and an all-gap row
    a = np.frombuffer(b"".join(family(rng, 7, 130)), np.uint8).reshape(7, 130).copy()
    a[:, [0, 63, 64, 129]] = ord("-")
    a[3, :] = ord("-")
    allgap = [r.tobytes() for r in a]
    # the highest count tied between three characters, the winner first seen in the last rows: 66 rows, so that the
    # three first occurrences fall to different waves; singletons above them
    n = 66
    t = np.full((n, 3), ord("-"), np.uint8)
    t[:57, 0] = np.arange(57) + 40                               # 57 singletons ('(' .. '`'), then z z y y x x z y x
    t[57:, 0] = np.frombuffer(b"zzyyxxzyx", np.uint8)
    t[:, 1] = t[::-1, 0]                                         # the same column upside down: x wins
    t[60:, 2] = np.frombuffer(b"CBAABC", np.uint8)               # C first, in row 60
    ties = [r.tobytes() for r in t]
    assert sr.columns(ties)["top_char"].tobytes() == b"zxC" and sr.columns(ties)["top_count"].tolist() == [3, 3, 2]
    # upper and lower case of one letter in one column
    case = [b"Aa", b"aA", b"AA", b"a-", b"Aa", b"aa"]
    # the bytes 0x01, 0x80 and 0xFF inside rows
    b = np.frombuffer(b"".join(family(rng, 5, 70, b"ACGU", 0.2)), np.uint8).reshape(5, 70).copy()
    b[1:3, 3] = 0x01
    b[[0, 4], 64] = 0x80
    b[2:5, 69] = 0xFF
    raw = [r.tobytes() for r in b]
    # a DNA-only family (both cases, N and U) and the same with one 'X'
    dna = family(rng, 12, 129, b"ACGTacgtNU", 0.2)
    one_x = [bytearray(r) for r in dna]
    one_x[7][100] = ord("X")
    one_x = [bytes(r) for r in one_x]
    assert sr.ambiguous(dna) == b"N" and sr.ambiguous(one_x) == b"X" and sr.ambiguous(raw) == b"X"
    check_batch(ctx, [allgap, ties, case, raw, dna, one_x], cons_thr=CONS_THR, gap_thr=GAP_THR)


def test_another_gap_byte(ctx):
    """'.' as the gap: '-' is then a character like any other"""
    rng = np.random.default_rng(5)
    fams = [family(rng, 6, 65, b"ACGT-", 0.3, gap=b"."), family(rng, 3, 64, b"ACGT", 0.3, gap=b".")]
    assert sr.ambiguous(fams[0], b".") == b"X" and sr.ambiguous(fams[1], b".") == b"N"
    check_batch(ctx, fams, gap=b".", cons_thr=CONS_THR, gap_thr=GAP_THR)
    check_batch(ctx, [family(rng, 4, 66, b"ACGT", 0.3, gap=b"\xff")], gap=b"\xff")


CASES = sorted(os.path.basename(p)[4:-4] for p in glob.glob(os.path.join(GOLDEN, "sum_*.npz")))


def _blocks(buf, n, widths):
    out, o = [], 0
    for w in widths:
        w = int(w)
        out.append([buf[o + r * w:o + (r + 1) * w].tobytes() for r in range(n)])
        o += n * w
    return out


def test_goldens_in_one_batch(ctx):
    """every recorded case as a family of one batch: the reference's numbers and strings from one handle"""
    from kalign_amd import summary
    zs = [np.load(os.path.join(GOLDEN, "sum_%s.npz" % c)) for c in CASES]
    fams = [[r.tobytes() for r in z["rows"]] for z in zs]
    assert len(fams) >= 15
    s = ctx.family_summary(fams)
    try:
        for d, z, name in zip(s.summary(), zs, CASES):
            assert [d["length"], d["n_sequences"]] == z["stats_i"].tolist(), name
            assert [d["gap_fraction"], d["conservation"], d["identity"]] == z["stats_f"].tolist(), name
        for k, t in enumerate(zs[0]["cons_thr"]):
            for got, z, name in zip(s.consensus(float(t)), zs, CASES):
                assert got == z["cons"][k].tobytes(), (name, t)
        for k, t in enumerate(zs[0]["rg_thr"]):
            for got, z, rows, name in zip(s.compact(float(t)), zs, fams, CASES):
                assert got == _blocks(z["rg"], len(rows), z["rg_w"])[k], (name, t)
        n_trim = min(len(z["trim_w"]) for z in zs)
        for k in range(n_trim):
            masks = []
            for z, rows in zip(zs, fams):
                w = len(rows[0])
                a, b = summary.trim_range(w, None if z["trim_none"][k, 0] else int(z["trim_arg"][k, 0]),
                                          None if z["trim_none"][k, 1] else int(z["trim_arg"][k, 1]))
                masks.append([int(a <= c < b) for c in range(w)])
            for got, z, rows, name in zip(s.compact(column_masks=masks), zs, fams, CASES):
                assert got == _blocks(z["trim"], len(rows), z["trim_w"])[k], (name, k)
    finally:
        s.close()


def test_fronts_with_the_reference_names(ctx):
    from kalign_amd import summary
    z = np.load(os.path.join(GOLDEN, "sum_syn_lower.npz"))
    aln = [r.tobytes().decode("latin-1") for r in z["rows"]]
    st = summary.alignment_stats(ctx, aln)
    assert list(st) == ["length", "n_sequences", "gap_fraction", "conservation", "identity"]
    assert [st["length"], st["n_sequences"]] == z["stats_i"].tolist()
    assert [st["gap_fraction"], st["conservation"], st["identity"]] == z["stats_f"].tolist()
    assert summary.consensus_sequence(ctx, aln, 2.0 / 3.0) == z["cons"][3].tobytes().decode("latin-1")
    assert summary.remove_gap_columns(ctx, aln, 0.25) == [r.decode("latin-1") for r in _blocks(z["rg"], len(aln), z["rg_w"])[1]]
    assert summary.trim_alignment(ctx, aln, 5, -5) == [r[5:-5] for r in aln]
    assert summary.remove_gap_columns(ctx, ["A-", "--"], 0.5) == ["", ""]
    # a str row is its latin-1 bytes on both ways in
    s = ctx.family_summary([["A\xe9-", "A\xe9C"]])
    assert s.consensus(0.5) == [b"A\xe9C"]
    s.close()
    assert summary.consensus_sequence(ctx, ["A\xe9-", "A\xe9C"]) == "A\xe9C"
    two = summary.consensus_sequences(ctx, [aln, ["ACGT", "ACGA", "AC-A"]], [0.5, 1.0])
    assert two == [z["cons"][2].tobytes().decode("latin-1"), "ACGN"]


def mixed_batch(rng, n_fam):
    """families of mixed sizes and widths, the smallest first and last"""
    fams = [[b"A"]]
    for k in range(n_fam - 2):
        n = int(rng.choice([1, 2, 3, 7, 9, 17, 40, 66]))
        w = int(rng.choice([1, 5, 63, 64, 65, 100, 130, 255, 256, 257, 300]))
        fams.append(family(rng, n, w, PROT if k % 2 else b"ACGTacgu", float(rng.choice([0.0, 0.3, 0.7]))))
    return fams + [[b"-"]]


def outputs(s):
    return (s.columns(), s.summary(), s.consensus(0.5, want_ambiguous=True), s.keep(0.5), s.compact(0.5), s.compact(1.0))


def test_a_family_in_a_batch_equals_the_family_alone(ctx):
    rng = np.random.default_rng(6)
    fams = mixed_batch(rng, 40)
    assert len(fams) == 40
    s = ctx.family_summary(fams)
    cols, summ, (cons, amb), kp, half, full = outputs(s)
    s.close()
    for f, rows in enumerate(fams):
        one = ctx.family_summary([rows])
        c1, s1, (k1, a1), p1, h1, f1 = outputs(one)
        one.close()
        for k in c1[0]:
            assert np.array_equal(c1[0][k], cols[f][k]), (f, k)
        assert s1[0] == summ[f] and k1[0] == cons[f] and a1[0] == amb[f], f
        assert np.array_equal(p1[0], kp[f]) and h1[0] == half[f] and f1[0] == full[f], f
    # ... and the restatement on a few of them (the smallest two among them)
    for f in (0, 1, 17, 38, 39):
        assert summ[f] == sr.summary(fams[f]) and cons[f] == sr.consensus(fams[f], 0.5) and half[f] == sr.compact(fams[f], 0.5), f


def test_launches_do_not_grow_with_the_batch(ctx):
    rng = np.random.default_rng(7)
    seen = []
    for n_fam in (3, 40):
        s = ctx.family_summary(mixed_batch(rng, n_fam))
        per_call = [("create", s.stats())]
        for name, call in (("consensus", s.consensus), ("keep", s.keep), ("compact", s.compact)):
            call()
            per_call.append((name, s.stats()))
            s.columns()                                           # (the hand-outs are copies: they do not count)
            s.summary()
            assert s.stats() == per_call[-1][1]
        s.close()
        seen.append([(name, st["launches"], st["syncs"]) for name, st in per_call])
    assert seen[0] == seen[1]
    launches = {name: n for name, n, _ in seen[0]}
    assert launches["create"] >= 1 and launches["consensus"] >= 1 and launches["compact"] > launches["keep"] >= 2
    assert all(syncs == 1 for _, _, syncs in seen[0])


def test_compaction(ctx):
    rng = np.random.default_rng(8)
    w = 600
    wide = family(rng, 3, w, gap_p=0.2)
    a = np.frombuffer(b"".join(wide), np.uint8).reshape(3, w)
    fams = [wide, family(rng, 4, 65), wide, wide]
    s = ctx.family_summary(fams)
    try:
        before = s.columns()
        ones = [np.ones(len(f[0]), np.int32) for f in fams]
        assert s.compact(column_masks=ones) == fams                                   # keep everything
        assert s.compact(0.0) == [[b""] * len(f) for f in fams]                       # keep nothing: no fraction is below 0
        assert s.compact(column_masks=[np.zeros(len(f[0]), np.int32) for f in fams]) == [[b""] * len(f) for f in fams]
        first = [np.eye(1, len(f[0]), 0, dtype=np.int32)[0] for f in fams]
        last = [np.eye(1, len(f[0]), len(f[0]) - 1, dtype=np.int32)[0] for f in fams]
        assert s.compact(column_masks=first) == [[r[:1] for r in f] for f in fams]
        assert s.compact(column_masks=last) == [[r[-1:] for r in f] for f in fams]
        # kept counts that cross the scan block's edge (256) by one, the kept columns spread over the width; family 1
        # by the gap rule in the same call
        masks = []
        for kept in (255, 256, 257):
            m = np.zeros(w, np.int32)
            m[np.sort(rng.choice(w, kept, replace=False))] = 7                        # (non-zero keeps)
            masks.append(m)
        masks = [masks[0], None, masks[1], masks[2]]
        got = s.compact(0.5, masks)
        kp = s.keep(0.5, masks)
        assert [len(f[0]) for f in got] == [255, int(sr.keep(fams[1], 0.5).sum()), 256, 257]
        for f in (0, 2, 3):
            assert got[f] == [a[r, masks[f] != 0].tobytes() for r in range(3)] and np.array_equal(kp[f], (masks[f] != 0).astype(np.int32))
        assert got[1] == sr.compact(fams[1], 0.5) and np.array_equal(kp[1], sr.keep(fams[1], 0.5))
        # the handle's rows are as they were: the table again from them, everything kept, and a second rule
        after = s.columns()
        for b, c in zip(before, after):
            assert all(np.array_equal(b[k], c[k]) for k in b)
        assert s.compact(column_masks=ones) == fams
        assert s.compact(1.0 / 3.0) == [sr.compact(f, 1.0 / 3.0) for f in fams]
        assert s.consensus(0.5) == [sr.consensus(f, 0.5) for f in fams]
    finally:
        s.close()


def test_a_refused_call_launches_nothing(ctx):
    from kalign_amd import KalignAmdError, api
    rng = np.random.default_rng(9)
    fams = [family(rng, 4, 70), family(rng, 2, 10), family(rng, 5, 130)]
    s = ctx.family_summary(fams)
    try:
        s.compact(0.5)                                            # (a call that launches, so that zeros below are the refusal's)
        assert s.stats()["launches"] > 0
        for call in (s.consensus, s.keep, s.compact):
            for bad in ([0.5, float("nan"), 0.5], [0.5, 0.5, 1.5], -0.1):
                with pytest.raises(KalignAmdError, match=r"ka_sum_fam_\w+: family \d: (gap )?threshold \S+ is not in \[0, 1\]"):
                    call(bad)
                st = s.stats()
                assert st["launches"] == 0 and st["syncs"] == 0
        # a mask offset past the end of the masks: through the C entry, the Python front packs its own offsets
        masks = np.ones(210, np.int32)
        off = np.array([0, -1, 81], np.int64)                     # 81 + 130 > 210 columns
        keep = np.full(210, -5, np.int32)
        for rc in (s.L.ka_sum_fam_keep(s.h, None, api._ptr(masks), api._ptr(off), api._ptr(keep), None),
                   s.L.ka_sum_fam_compact(s.h, None, api._ptr(masks), api._ptr(off), None)):
            assert rc != 0
            assert "family 2: mask offset 81 with 130 columns passes the end of the masks (210 ints at most)" in s.L.ka_last_error().decode()
            st = s.stats()
            assert st["launches"] == 0 and st["syncs"] == 0
        assert (keep == -5).all()
        # ... and the handle is as usable as before
        assert s.consensus(0.5) == [sr.consensus(f, 0.5) for f in fams] and s.stats()["launches"] > 0
        assert s.compact(0.5) == [sr.compact(f, 0.5) for f in fams]
        off[2] = 80
        assert s.L.ka_sum_fam_keep(s.h, None, api._ptr(masks), api._ptr(off), api._ptr(keep), None) == 0
        assert np.array_equal(keep[80:], np.ones(130, np.int32)) and np.array_equal(keep[70:80], sr.keep(fams[1]))
    finally:
        s.close()
    with pytest.raises(KalignAmdError, match="ka_sum_fam_create: family 1: alnlen 0"):
        ctx.family_summary([["AC"], [""]])
    with pytest.raises(KalignAmdError, match="ka_sum_fam_create: empty family"):
        ctx.family_summary([["AC"], []])


def test_keep_is_a_column_mask_of_compare_families(ctx):
    """keep()'s list goes into compare_families as it stands: the scores of the comparer with that mask"""
    from kalign_amd import compare
    z = np.load(os.path.join(GOLDEN, "cmp_syn_gapfrac5.npz"))
    ref, test = [str(r) for r in z["ref"]], [str(r) for r in z["tests"][0]]
    z2 = np.load(os.path.join(GOLDEN, "cmp_syn_prot24.npz"))
    ref2, test2 = [str(r) for r in z2["ref"]], [str(r) for r in z2["tests"][1]]
    s = ctx.family_summary([ref, ref2])
    kp = s.keep(0.25)
    s.close()
    assert 0 < int(kp[0].sum()) < len(ref[0]) and np.array_equal(kp[0], sr.keep(ref, 0.25))
    got = compare.compare_families(ctx, [ref, ref2], [test, test2], column_masks=kp)
    for g, (r, t, m) in zip(got, ((ref, test, kp[0]), (ref2, test2, kp[1]))):
        assert g == compare.compare(ctx, r, t, column_mask=m)
