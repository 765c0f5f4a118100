"""GPU: the output stage (ka_out_fam; Context.family_output, kalign_amd.output) against the Python restatement
(tests/out_restate.py) and against the goldens recorded from the reference (tests/golden/out_*.npz): every text compared
with == on bytes, no tolerance.

The fill kernel writes a dword a lane, 256 bytes a wave and 1024 a workgroup, and a dword is assembled from as many lines as
it spans: with names of every length from 1 to 255 and lines of 1 to 513 columns, line ends fall on every byte of a dword and
family ends inside waves and workgroups.  The blocks of Clustal and MSF are 60 columns: widths stand at 1 and around 60 and
120.  The MSF row pass walks a row 256 columns a step as four ballots of 64: widths stand around 64, 256 and 512, and the
checksum's prefix ends inside, at and past the first step and around the weights' wrap at 57.  The row pass deals four rows
to a workgroup: families of 1 .. 5 and 15, 16, 17 rows put the end of one family and the start of the next inside one."""
import os
import re

import numpy as np
import pytest

import out_restate as orr
from util import GOLDEN

pytestmark = pytest.mark.gpu

WIDTHS = [1, 59, 60, 61, 119, 120, 121, 63, 64, 65, 255, 256, 257, 513]
SIZES = [1, 2, 3, 4, 5, 15, 16, 17, 2, 3, 1, 2, 3, 4]
LINE_LENGTHS = [1, 7, 60, 80, 61, 62, 119, 120, 121, 512, 513, 514]      # W - 1, W, W + 1 of the families of 61, 120 and 513 columns
DATE = b"October 03, 1996 15:57"
G = {g.name: g for g in orr.goldens(GOLDEN)}
LETTERS = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWYacdxyz*-.--", np.uint8)


@pytest.fixture(scope="module")
def ctx():
    import kalign_amd
    c = kalign_amd.Context(0)
    yield c
    c.close()


def make_batch():
    rng = np.random.default_rng(20261021)
    fams, names = [], []
    for n, w in zip(SIZES, WIDTHS):
        fams.append([rng.choice(LETTERS, size=w).tobytes() for _ in range(n)])
        names.append([bytes(rng.integers(33, 127, int(k)).astype(np.uint8)) for k in rng.integers(1, 40, n)])
    # names of 1 and 255 bytes in one family: the longest first, last and in the middle
    names[5][0], names[5][7], names[5][14] = b"F" * 255, b"m", b"L" * 255
    names[6][0], names[6][8] = b"s", b"M" * 255
    names[7][16] = b"E" * 255
    names[1] = [b"a b", b" "]                                     # (a space is printable)
    assert any(b"." in r for f in fams for r in f) and any(b"-" in r for f in fams for r in f)
    return fams, names


BATCH, NAMES = make_batch()


@pytest.fixture(scope="module")
def out(ctx):
    h = ctx.family_output(BATCH, NAMES)
    yield h
    h.close()


@pytest.fixture(scope="module")
def out_unnamed(ctx):
    h = ctx.family_output(BATCH)
    yield h
    h.close()


def confidences(seed=7):
    """float32 confidences of the batch with the recorded sweep at the first and the last columns of a row and across the
    columns 255 | 256 of the wide families"""
    rng = np.random.default_rng(seed)
    sw = G["pp"].z["values"]
    res = [rng.random((n, w)).astype(np.float32) for n, w in zip(SIZES, WIDTHS)]
    col = [rng.random(w).astype(np.float32) for w in WIDTHS]
    for f, w in enumerate(WIDTHS):
        k = min(len(sw), w)
        res[f][0, :k], res[f][-1, w - k:] = sw[:k], sw[:k][::-1]
        col[f][:k] = sw[:k][::-1]
        col[f][-1] = sw[6]
        if w > 257:
            res[f][1, 256 - 17:256 + 17], col[f][256 - 17:256 + 17] = sw, sw
    return res, col


def test_fasta(out, out_unnamed):
    for L in LINE_LENGTHS:
        got = out.fasta(L)
        assert got == [orr.fasta(r, n, L) for r, n in zip(BATCH, NAMES)], L
        assert out.stats()["launches"] == 1 and out.stats()["syncs"] == 1
    assert out.fasta() == [orr.fasta(r, n, 60) for r, n in zip(BATCH, NAMES)]
    for L in (60, 80):
        assert out_unnamed.fasta(L) == [orr.fasta(r, None, L) for r in BATCH], L
    from kalign_amd import api
    with pytest.raises(api.KalignAmdError, match="ka_out_fam_fasta_size: line_length 0; a line holds one column at least"):
        out.fasta(0)


def test_clustal(out, out_unnamed):
    from kalign_amd import api
    assert out.clustal() == [orr.clustal(r, n, api.CLUSTAL_HEADER) for r, n in zip(BATCH, NAMES)]
    for hd in (b"", b"x", b"CLUSTAL W (1.83) multiple sequence alignment", b"h" * 255):
        assert out.clustal(hd) == [orr.clustal(r, n, hd) for r, n in zip(BATCH, NAMES)], hd
    assert out_unnamed.clustal() == [orr.clustal(r, None, api.CLUSTAL_HEADER) for r in BATCH]
    with pytest.raises(api.KalignAmdError, match="ka_out_fam_clustal_size: header of 256 bytes; it holds 255 at most"):
        out.clustal(b"h" * 256)


def msf_family(W, counts):
    """rows of W columns with these character counts, characters and gaps mixed (the last row: no gap)"""
    rng = np.random.default_rng(W)
    rows = []
    for n in counts:
        r = np.full(W, ord("-"), np.uint8)
        r[rng.choice(W, size=n, replace=False)] = rng.choice(np.frombuffer(b"ACDEFGHIKLMNPQRSTVWYacdwy", np.uint8), size=n)
        rows.append(r.tobytes())
    return rows


def test_msf_records_and_text(ctx):
    # character counts 0 (an all-gap row), 1, 56, 57, 58 and W: the weight's wrap at 57; a prefix ending inside, at and past
    # the first step of 256 columns
    fams = [msf_family(300, [0, 1, 56, 57, 58, 255, 256, 257, 300]), msf_family(58, [58, 57, 56, 1, 0]), msf_family(513, [512, 513, 0, 511]),
            [b"W" * 64] * 5]
    names = [[b"r%d" % i for i in range(len(f))] for f in fams]
    names[1][0] = b"all of it"
    h = ctx.family_output(fams, names)
    try:
        want = [orr.msf_records(f) for f in fams]
        assert want[0][0][0] == (0, 0) and [c for c, _ in want[0][0]] == [0, 1, 56, 57, 58, 255, 256, 257, 300]
        assert sum(c for _, c in want[3][0]) > 10000 and want[3][1] == sum(c for _, c in want[3][0]) % 10000   # the checks sum past 10000
        titles, bts = [b"a.msf", b"stdout", b"some name.msf", b"d"], [0, 1, 0, 1]
        first = h.msf(titles, bts, DATE)
        st = h.stats()
        assert (st["launches"], st["syncs"]) == (2, 2)                      # the row pass, then the fill
        assert first == [orr.msf(f, n, t, b, DATE) for f, n, t, b in zip(fams, names, titles, bts)]
        assert b" Name: r0  Len:      0  Check:    0  Weight: 1.00\n" in first[0] and b"  MSF: 0  Type: N  " in first[0]
        for (recs, check), (wr, wc) in zip(h.msf_records(), want):
            assert recs.dtype == np.int32 and [tuple(int(x) for x in r) for r in recs] == wr and check == wc
        again = h.msf(titles[::-1], 1, b"January 01, 2027 00:00")
        st = h.stats()
        assert (st["launches"], st["syncs"]) == (1, 1)                      # the records are the handle's
        assert again == [orr.msf(f, n, t, 1, b"January 01, 2027 00:00") for f, n, t in zip(fams, names, titles[::-1])]
        assert st["rows_ms"] > 0 and st["fill_ms"] > 0
    finally:
        h.close()


def test_msf_of_the_batch(out, out_unnamed):
    from kalign_amd import api
    titles = [b"fam%d.msf" % f for f in range(len(BATCH))]
    bts = [f & 1 for f in range(len(BATCH))]
    assert out.msf(titles, bts, DATE) == [orr.msf(r, n, t, b, DATE) for r, n, t, b in zip(BATCH, NAMES, titles, bts)]
    # records first, then the writer: the row pass counts with the first writer after it
    recs = out_unnamed.msf_records()
    assert [([tuple(int(x) for x in r) for r in a], c) for a, c in recs] == [orr.msf_records(r) for r in BATCH]
    assert out_unnamed.msf(titles, 0, DATE) == [orr.msf(r, None, t, 0, DATE) for r, t in zip(BATCH, titles)]
    st = out_unnamed.stats()
    assert (st["launches"], st["syncs"]) == (2, 2)
    for bad, msg in (((titles[:-1] + [b""], 0, DATE), "ka_out_fam_msf_size: family 13: title of 0 bytes; it holds 1 to 255"),
                     ((titles[:-1] + [b"a\tb"], 0, DATE), "ka_out_fam_msf_size: family 13: title holds a byte that is not printable ASCII (32..126)"),
                     ((titles, 2, DATE), "ka_out_fam_msf_size: family 0: biotype 2 is not 0 (protein) or 1 (DNA)"),
                     ((titles, 0, b""), "ka_out_fam_msf_size: the date of 0 bytes; it holds 1 to 63"),
                     ((titles, 0, b"d" * 64), "ka_out_fam_msf_size: the date of 64 bytes; it holds 1 to 63")):
        with pytest.raises(api.KalignAmdError, match=re.escape(msg)):
            out.msf(*bad)
    # the date is now's when none is given: the text differs from a dated one in that field alone
    import time
    lo = time.strftime(api.MSF_DATE).encode()
    got = out.msf(titles, bts)
    hi = time.strftime(api.MSF_DATE).encode()
    assert got in ([orr.msf(r, n, t, b, d) for r, n, t, b in zip(BATCH, NAMES, titles, bts)] for d in (lo, hi))


def test_stockholm(out, out_unnamed):
    res, col = confidences()
    for r, c in ((res, None), (None, col), (res, col)):
        got = out.stockholm(r, c)
        want = [orr.stockholm(rows, n, None if r is None else r[f], None if c is None else c[f]) for f, (rows, n) in enumerate(zip(BATCH, NAMES))]
        assert got == want
        st = out.stats()
        assert (st["launches"], st["syncs"]) == (1, 1)
    assert out_unnamed.stockholm(res, col) == [orr.stockholm(rows, None, res[f], col[f]) for f, rows in enumerate(BATCH)]
    # float32 values in float64 arrays pass; lists of lists pass
    assert out.stockholm([x.astype(np.float64) for x in res], [x.tolist() for x in col]) == \
        [orr.stockholm(rows, n, res[f], col[f]) for f, (rows, n) in enumerate(zip(BATCH, NAMES))]
    from kalign_amd import api
    with pytest.raises(api.KalignAmdError, match="ka_out_fam_stockholm_size: without confidences the reference writes Stockholm through Biopython"):
        out.stockholm()


def test_stockholm_refuses_a_confidence_outside_the_range(out):
    from kalign_amd import api
    res, col = confidences(9)
    want = [orr.stockholm(rows, n, res[f], col[f]) for f, (rows, n) in enumerate(zip(BATCH, NAMES))]
    f, s, c = 6, 9, 5

    def at_character(f, s):
        return next(k for k, b in enumerate(BATCH[f][s]) if b not in b"-.")
    c = at_character(f, s)
    for v, shown in ((np.nan, "nan"), (-0.001, "-0.00100000005"), (1.0001, "1.00010002")):
        bad = [x.copy() for x in res]
        bad[f][s, c] = v
        # a later offender, a column offender of an earlier family's successor and one under a gap: the first in batch order is named
        bad[9][1, at_character(9, 1)] = 2.0
        gap_col = next(k for k, b in enumerate(BATCH[2][0]) if b in b"-.") if any(b in b"-." for b in BATCH[2][0]) else None
        if gap_col is not None:
            bad[2][0, gap_col] = np.nan                          # (under a gap: not looked at, as in the reference)
        with pytest.raises(api.KalignAmdError, match=re.escape("ka_out_fam_stockholm: family %d, sequence %d, column %d: confidence %s outside [0, 1]" % (f, s, c, shown))):
            out.stockholm(bad, col)
        assert out.stockholm(res, col) == want                   # the handle is still good
    badc = [x.copy() for x in col]
    badc[3][60] = 1.5
    badr = [x.copy() for x in res]
    badr[4][0, at_character(4, 0)] = -1.0                        # a later family's residue comes after family 3's column
    with pytest.raises(api.KalignAmdError, match=re.escape("ka_out_fam_stockholm: family 3, column 60: column confidence 1.5 outside [0, 1]")):
        out.stockholm(badr, badc)
    with pytest.raises(api.KalignAmdError, match=re.escape("ka_out_fam_stockholm: family 3, column 60: column confidence 1.5 outside [0, 1]")):
        out.stockholm(None, badc)
    assert out.stockholm(None, col) == [orr.stockholm(rows, n, None, col[k]) for k, (rows, n) in enumerate(zip(BATCH, NAMES))]


def test_the_goldens_through_the_device(ctx):
    from kalign_amd import api
    cases = [G["prot"], G["dna"], G["w120"]]
    h = ctx.family_output([g.rows for g in cases], [g.names for g in cases])
    try:
        assert h.fasta(60) == [g.text("fasta") for g in cases]
        assert h.clustal() == [g.text("clu") for g in cases]
        # the date is a call's: the cases were recorded within a minute or two of each other, each text under its own
        for k, g in enumerate(cases):
            assert h.msf([c.text("title") for c in cases], [int(c.z["biotype"]) for c in cases], g.text("date"))[k] == g.text("msf"), g.name
    finally:
        h.close()
    two = cases[:2]
    h = ctx.family_output([g.rows for g in two], [g.names for g in two])
    try:
        assert h.fasta(80) == [g.text("fasta80") for g in two] and h.fasta(7) == [g.text("fasta7") for g in two]
        res, col = [g.z["residue_conf"] for g in two], [g.z["column_conf"] for g in two]
        assert h.stockholm(res, None) == [g.text("sto_res") for g in two]
        assert h.stockholm(None, col) == [g.text("sto_col") for g in two]
        assert h.stockholm(res, col) == [g.text("sto_both") for g in two]
    finally:
        h.close()
    h = ctx.family_output([g.rows for g in two])
    try:
        assert h.stockholm([g.z["residue_conf"] for g in two], [g.z["column_conf"] for g in two]) == [g.text("sto_noids") for g in two]
    finally:
        h.close()
    assert api.CLUSTAL_HEADER in cases[0].text("clu")


@pytest.mark.parametrize("n_fam", [1, 40])
def test_launches_and_synchronisations_do_not_grow_with_the_batch(ctx, n_fam):
    rng = np.random.default_rng(n_fam)
    fams = [[rng.choice(LETTERS, size=50 + f).tobytes() for _ in range(1 + f % 5)] for f in range(n_fam)]
    res = [rng.random((len(r), len(r[0]))).astype(np.float32) for r in fams]
    h = ctx.family_output(fams)
    try:
        counts = {}
        for name, call in (("fasta", lambda: h.fasta(80)), ("clustal", h.clustal), ("stockholm", lambda: h.stockholm(res)),
                           ("msf", lambda: h.msf([b"t"] * n_fam, 0, DATE)), ("msf again", lambda: h.msf([b"t"] * n_fam, 1, DATE))):
            assert len(call()) == n_fam
            st = h.stats()
            counts[name] = (st["launches"], st["syncs"])
        assert counts == {"fasta": (1, 1), "clustal": (1, 1), "stockholm": (1, 1), "msf": (2, 2), "msf again": (1, 1)}
    finally:
        h.close()


def test_a_cap_one_byte_short_is_refused_before_the_fill(ctx):
    from kalign_amd import api
    fams, names = BATCH[:4], NAMES[:4]
    h = ctx.family_output(fams, names)
    try:
        assert h.stats()["launches"] == 0
        res = [np.zeros((len(r), len(r[0])), np.float32) for r in fams]
        size = {"fasta": sum(len(orr.fasta(r, n, 60)) for r, n in zip(fams, names)),
                "clustal": sum(len(orr.clustal(r, n, api.CLUSTAL_HEADER)) for r, n in zip(fams, names)),
                "stockholm": sum(len(orr.stockholm(r, n, x, None)) for r, n, x in zip(fams, names, res))}
        for name, call in (("fasta", lambda cap: h.fasta(60, cap=cap)), ("clustal", lambda cap: h.clustal(cap=cap)),
                           ("stockholm", lambda cap: h.stockholm(res, cap=cap))):
            with pytest.raises(api.KalignAmdError, match=re.escape("ka_out_fam_%s: %d bytes do not hold the text (%d)" % (name, size[name] - 1, size[name]))):
                call(size[name] - 1)
            st = h.stats()
            assert st["launches"] == 0 and st["syncs"] == 0 and st["fill_ms"] == 0     # nothing has been launched
        # MSF's size needs the records: the row pass runs, the fill does not
        size = sum(len(orr.msf(r, n, b"t", 0, DATE)) for r, n in zip(fams, names))
        with pytest.raises(api.KalignAmdError, match=re.escape("ka_out_fam_msf: %d bytes do not hold the text (%d)" % (size - 1, size))):
            h.msf([b"t"] * 4, 0, DATE, cap=size - 1)
        assert h.stats()["fill_ms"] == 0
        assert h.fasta(60, cap=size + 100) == [orr.fasta(r, n, 60) for r, n in zip(fams, names)]   # a larger cap is fine; the handle is good
    finally:
        h.close()


def test_gap_byte_and_character_rule(ctx):
    # the handle's gap decides MSF's characters alone; Stockholm's '.' goes by '-' and '.', whatever the gap
    rows = [[b"AC.-x", b".....", b"a-c-e"]]
    h = ctx.family_output(rows, gap=b".")
    try:
        recs, check = h.msf_records()[0]
        assert [tuple(int(x) for x in r) for r in recs] == orr.msf_records(rows[0], b".")[0] and [int(r[0]) for r in recs] == [4, 0, 5]
        res = [np.full((3, 5), 0.5, np.float32)]
        assert h.stockholm(res)[0] == orr.stockholm(rows[0], None, res[0]) and b"PP 55..5\n" in h.stockholm(res)[0]
    finally:
        h.close()


def test_output_module(ctx, tmp_path):
    from kalign_amd import api, output
    fams, names = BATCH[:5], NAMES[:5]
    assert output.format_families(ctx, fams, names, "fasta", line_length=80) == [orr.fasta(r, n, 80) for r, n in zip(fams, names)]
    assert output.format_families(ctx, fams, None, "clustal") == [orr.clustal(r, None, api.CLUSTAL_HEADER) for r in fams]
    assert output.format_alignment(ctx, fams[4], names[4], "msf", title=b"one.msf", biotype=1, date=DATE) == orr.msf(fams[4], names[4], b"one.msf", 1, DATE)
    res, col = confidences()
    assert output.format_alignment(ctx, fams[3], names[3], "stockholm", residue_confidence=res[3], column_confidence=col[3]) == \
        orr.stockholm(fams[3], names[3], res[3], col[3])
    paths = [tmp_path / ("family_%d.msf" % f) for f in range(5)]
    texts = output.write_families(ctx, fams, names, "msf", paths, biotypes=0, date=DATE)
    for f, p in enumerate(paths):
        assert p.read_bytes() == texts[f] == orr.msf(fams[f], names[f], os.path.basename(str(p)).encode(), 0, DATE)
    results = [dict(rows=r, residue_confidence=res[f], column_confidence=col[f]) for f, r in enumerate(fams)]
    assert output.stockholm_families(ctx, results, names) == [orr.stockholm(r, n, res[f], col[f]) for f, (r, n) in enumerate(zip(fams, names))]
    with pytest.raises(api.KalignAmdError, match="is not a float32 value"):
        output.stockholm_families(ctx, [dict(rows=fams[0], residue_confidence=np.full((1, 1), 0.95), column_confidence=col[0])], None)
    with pytest.raises(api.KalignAmdError, match="format 'phylip' is not one of"):
        output.format_families(ctx, fams, names, "phylip")
