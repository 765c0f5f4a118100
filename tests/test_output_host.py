"""The host side of the output stage (ka_out_*): the names and the ABI revision; ka_out_fam_check's refusals; the closed-form
sizes (ka_out_fam_text_sizes) and the PP rule (ka_out_pp_char) -- the library's host-only functions -- and the Python
restatement (tests/out_restate.py) against every golden recorded from the reference (tests/golden/out_*.npz,
tests/golden/make_output_golden.py); output.py's float64 refusal.  No GPU, no tolerance: every comparison is ==."""
import os
import re

import numpy as np
import pytest

import out_restate as orr
from util import GOLDEN

NAMES = ("ka_out_pp_char", "ka_out_fam_check", "ka_out_fam_text_sizes", "ka_out_fam_create", "ka_out_fam_destroy", "ka_out_fam_fasta_size",
         "ka_out_fam_fasta", "ka_out_fam_clustal_size", "ka_out_fam_clustal", "ka_out_fam_msf_records", "ka_out_fam_msf_size", "ka_out_fam_msf",
         "ka_out_fam_stockholm_size", "ka_out_fam_stockholm", "ka_out_fam_stats")
G = orr.goldens(GOLDEN)


def by_name(name):
    return next(g for g in G if g.name == name)


def test_names_and_version():
    import kalign_amd
    from kalign_amd import api, output
    L = kalign_amd.load_library()
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "kalign_amd.h")).read()
    declared = set(re.findall(r"\b(ka_[a-z_]+)\s*\(", hdr))
    for name in NAMES:
        assert name in declared and name in api.EXPORTS and hasattr(L, name), name
    assert L.ka_abi_version() >= 30
    for m in ("fasta", "clustal", "msf", "msf_records", "stockholm", "stats"):
        assert callable(getattr(api.FamilyOutput, m)), m
    assert callable(api.Context.family_output)
    for m in ("format_families", "format_alignment", "write_families", "stockholm_families"):
        assert callable(getattr(output, m)), m
    assert kalign_amd.output is output
    assert api.OUT_STATS == ("rows_ms", "fill_ms", "launches", "syncs")


def test_the_cases_are_there():
    assert {"prot", "dna", "w120", "pp"} <= {g.name for g in G}
    for k, bt in (("prot", 0), ("dna", 1)):
        g = by_name(k)
        lens = [len(n) for n in g.names]
        assert int(g.z["biotype"]) == bt and len(set(lens)) > 1 and lens[0] != max(lens) and any(b" " in n for n in g.names)
        assert b"-" in b"".join(g.rows)
        for key in ("fasta", "clu", "msf", "fasta80", "fasta7", "sto_res", "sto_col", "sto_both", "sto_noids", "residue_conf", "column_conf"):
            assert g.has(key), (k, key)
    g = by_name("w120")
    assert len(g.rows[0]) == 120 and all(b"-" not in r for r in g.rows)              # the multiple-of-60 edge: no empty block
    assert g.text("clu").count(b"\n\n\n") == 2
    for g in G:
        assert os.path.getsize(os.path.join(GOLDEN, "out_%s.npz" % g.name)) < 16384


def test_restatement_equals_every_golden():
    from kalign_amd import api
    n = 0
    for g in G:
        if g.rows is None:
            continue
        bt = int(g.z["biotype"])
        assert orr.fasta(g.rows, g.names, 60) == g.text("fasta"), g.name
        assert orr.clustal(g.rows, g.names, api.CLUSTAL_HEADER) == g.text("clu"), g.name     # (pins the header's version)
        assert orr.msf(g.rows, g.names, g.text("title"), bt, g.text("date")) == g.text("msf"), g.name
        n += 3
        if not g.has("fasta80"):
            continue
        res, col = g.z["residue_conf"], g.z["column_conf"]
        assert res.dtype == np.float32 and col.dtype == np.float32
        assert orr.fasta(g.rows, g.names, 80) == g.text("fasta80") and orr.fasta(g.rows, g.names, 7) == g.text("fasta7"), g.name
        assert orr.stockholm(g.rows, g.names, res, None) == g.text("sto_res"), g.name
        assert orr.stockholm(g.rows, g.names, None, col) == g.text("sto_col"), g.name
        assert orr.stockholm(g.rows, g.names, res, col) == g.text("sto_both"), g.name
        assert orr.stockholm(g.rows, None, res, col) == g.text("sto_noids"), g.name
        n += 6
    assert n == 21


def test_what_the_reference_writes_for_both_biotypes():
    """banner and type letter are the same for a protein and a DNA family: what the header states"""
    for k in ("prot", "dna", "w120"):
        lines = by_name(k).text("msf").split(b"\n")
        assert lines[0] == b"!!NA_MULTIPLE_ALIGNMENT 1.0" and b"  Type: N  " in lines[2], k
    # MSF: and Len: carry the characters of row 0, not the width
    g = by_name("prot")
    chars0 = len(g.rows[0]) - g.rows[0].count(b"-")
    assert chars0 < len(g.rows[0]) and (b"  MSF: %d  " % chars0) in g.text("msf") and g.text("msf").count(b"Len:  %5d" % chars0) == len(g.rows)


def test_pp_char_on_the_recorded_sweep():
    from kalign_amd import api
    z = by_name("pp").z
    values, chars = z["values"], z["chars"].tobytes()
    assert values.dtype == np.float32 and len(values) == len(chars) == 34
    f = np.float32
    for v in (f(0), f(1), np.nextafter(f(0.95), f(0)), np.nextafter(f(0.95), f(1)), f(1e-42)):
        assert v in values
    assert any(v == 0 and np.signbit(v) for v in values)
    for k in range(1, 10):
        e = f(k / 10)
        assert np.nextafter(e, f(0)) in values and np.nextafter(e, f(1)) in values
    for v, c in zip(values, chars):
        assert api.pp_char(v) == bytes([c]) == orr.pp_char(v), v
    for v in (np.nan, -0.001, 1.0001, np.inf, -np.inf, np.nextafter(f(1), f(2)), -1e-45):
        assert api.pp_char(v) is None and orr.pp_char(v) is None, v


def refused(rows, names, match):
    from kalign_amd import api
    with pytest.raises(api.KalignAmdError, match=re.escape(match)):
        api.output_check(rows, names)


def test_check_refusals():
    from kalign_amd import api
    rows = [[b"AC-", b"A-C"], [b"ACGT", b"AC-T", b"A--T"]]
    ok = [[b"a", b"b"], [b"x" * 255, b" ~", b"c"]]
    api.output_check(rows, ok)                                   # 255 bytes, 32 and 126 pass
    api.output_check(rows, None)

    def with_name(n):
        return [[b"a", b"b"], [b"x", b"y", n]]
    refused(rows, with_name(b"ab\x1fc"), "ka_out_fam_check: family 1, sequence 2: name byte 0x1f at offset 2; a name is printable ASCII (32..126)")
    refused(rows, with_name(b"\x7f"), "ka_out_fam_check: family 1, sequence 2: name byte 0x7f at offset 0; a name is printable ASCII (32..126)")
    refused(rows, with_name(b"abc\xc8"), "ka_out_fam_check: family 1, sequence 2: name byte 0xc8 at offset 3; a name is printable ASCII (32..126)")
    refused(rows, with_name(b""), "ka_out_fam_check: family 1, sequence 2: empty name")
    refused(rows, with_name(b"x" * 256), "ka_out_fam_check: family 1, sequence 2: name of 256 bytes; a name holds 1 to 255")
    refused(rows, [[b"a", b""], [b"x", b"y", b"z"]], "ka_out_fam_check: family 0, sequence 1: empty name")
    # the batch rules are ka_sum_fam_check's, under this stage's name
    refused([[b"AC"], []], None, "ka_out_fam_check: empty family")
    refused([[b"", b""]], None, "ka_out_fam_check: family 0: alnlen 0")
    import ctypes as C
    L = api.load_library()

    def raw(n_fam, first, alnlens):
        f, a, r = np.ascontiguousarray(first, np.int32), np.ascontiguousarray(alnlens, np.int32), np.zeros(8, np.uint8)
        vp = C.c_void_p
        rc = L.ka_out_fam_check(n_fam, f.ctypes.data_as(vp), r.ctypes.data_as(vp), a.ctypes.data_as(vp), None, None)
        return rc, L.ka_last_error().decode()
    assert raw(0, [0], [1]) == (1, "ka_out_fam_check: bad arguments")
    assert raw(2, [1, 2, 3], [1, 1]) == (1, "ka_out_fam_check: fam_first does not ascend from 0 to numseq")
    assert raw(2, [0, 2, 1], [1, 1]) == (1, "ka_out_fam_check: fam_first does not ascend from 0 to numseq")
    assert raw(1, [0, 2], [2 ** 31 - 1]) == (1, "ka_out_fam_check: family 0: 2 rows of 2147483647 columns; a family holds fewer than 2^31 cells")


def shapes():
    rng = np.random.default_rng(11)
    sizes = [1, 2, 3, 4, 5, 15, 16, 17, 2, 3, 1, 2, 3, 4]
    widths = [1, 59, 60, 61, 119, 120, 121, 63, 64, 65, 255, 256, 257, 513]
    lens = [[int(x) for x in rng.integers(1, 256, n)] for n in sizes]
    lens[5][0], lens[5][7], lens[5][14] = 255, 1, 255
    return sizes, widths, lens


def test_closed_form_sizes_equal_the_restatement():
    from kalign_amd import api
    sizes, widths, lens = shapes()
    fams = [[b"A" * w] * n for n, w in zip(sizes, widths)]
    names = [[b"n" * k for k in f] for f in lens]
    for L in (1, 7, 60, 80, 512, 513, 514):
        got = api.output_sizes(sizes, widths, lens, "fasta", L)
        assert got.tolist() == [len(orr.fasta(r, n, L)) for r, n in zip(fams, names)] == [orr.fasta_size((w, f), L) for w, f in zip(widths, lens)], L
    hd = api.CLUSTAL_HEADER
    got = api.output_sizes(sizes, widths, lens, "clustal", len(hd))
    assert got.tolist() == [len(orr.clustal(r, n, hd)) for r, n in zip(fams, names)] == [len(hd) + 2 + orr.blocks_size(w, f) for w, f in zip(widths, lens)]
    for param, (has_res, has_col) in ((1, (True, False)), (2, (False, True)), (3, (True, True))):
        got = api.output_sizes(sizes, widths, lens, "stockholm", param)
        want = []
        for r, n in zip(fams, names):
            res = np.zeros((len(r), len(r[0])), np.float32) if has_res else None
            col = np.zeros(len(r[0]), np.float32) if has_col else None
            want.append(len(orr.stockholm(r, n, res, col)))
        assert got.tolist() == want == [orr.stockholm_size(w, f, has_res, has_col) for w, f in zip(widths, lens)], param
    # the default names: seq0, seq1, ...
    got = api.output_sizes(sizes, widths, None, "clustal", 0)
    assert got.tolist() == [len(orr.clustal(r, None, b"")) for r in fams]
    assert api.output_sizes([12], [70], None, "fasta", 60).tolist() == [len(orr.fasta([b"A" * 70] * 12, None, 60))]
    for fmt, param, msg in (("fasta", 0, "ka_out_fam_text_sizes: line_length 0; a line holds one column at least"),
                            ("clustal", 256, "ka_out_fam_text_sizes: header of 256 bytes; it holds 255 at most"),
                            ("stockholm", 0, "ka_out_fam_text_sizes: confidences 0 are not 1 (residue), 2 (column) or 3 (both)")):
        with pytest.raises(api.KalignAmdError, match=re.escape(msg)):
            api.output_sizes(sizes, widths, lens, fmt, param)


def test_restatement_by_hand():
    # a width that is a multiple of 60 opens no empty block; one column more opens a block of one
    rows, names = [b"A" * 60, b"C" * 60], [b"x", b"yyy"]
    assert orr.clustal(rows, names, b"H") == b"H\n\nx       " + b"A" * 60 + b"\nyyy     " + b"C" * 60 + b"\n\n\n"
    rows = [b"A" * 61, b"C" * 61]
    assert orr.clustal(rows, names, b"H").endswith(b"\n\n\nx       A\nyyy     C\n\n\n")
    assert orr.fasta([b"ACGTA"], [b"s"], 2) == b">s\nAC\nGT\nA\n" and orr.fasta([b"ACGT"], None, 2) == b">seq0\nAC\nGT\n"
    # MSF: an all-gap row has no character and checks 0; a prefix holds gaps; the weights wrap at 57
    recs, check = orr.msf_records([b"--A-c", b"-----", b"ACGTA"])
    assert recs == [(2, (1 * 45 + 2 * 45) % 10000), (0, 0), (5, sum((i + 1) * c for i, c in enumerate(b"ACGTA")) % 10000)]
    assert check == sum(c for _, c in recs) % 10000
    assert orr.msf_records([b"a" * 58])[0] == [(58, (65 * (57 * 58 // 2) + 65) % 10000)]
    text = orr.msf([b"-----", b"AC-GT"], [b"gap", b"s"], b"stdout", 0, b"October 03, 1996 15:57")
    assert text.split(b"\n")[2] == b" stdout  MSF: 0  Type: N  October 03, 1996 15:57  Check: %d  .." % orr.msf_records([b"AC-GT"])[1]
    assert b" Name: gap  Len:      0  Check:    0  Weight: 1.00\n" in text
    assert orr.stockholm([b"A-.C"], [b"s"], np.array([[0.96, 0.0, 0.0, 0.949]], np.float32), np.array([1, 0, 0.5, 0.09], np.float32)) == \
        b"# STOCKHOLM 1.0\ns   A-.C\n#=GR s PP *..9\n#=GC PP_cons   *050\n//\n"


def test_float64_confidences_must_be_float32_values():
    """kalign_amd.api.FamilyOutput._conf (what output.py hands confidences through): a float64 array is taken only when every
    value survives the round trip to float32"""
    from kalign_amd import api
    conv = api.FamilyOutput._conf
    me = type("Shape", (), dict(sizes=[2], widths=np.array([3], np.int32)))()
    exact = np.array([[0.5, 0.25, 1.0], [0.0, np.nan, 0.75]], np.float64)
    got = conv(me, [exact], True, "residue")
    assert got.dtype == np.float32 and np.array_equal(got, exact.astype(np.float32).reshape(-1), equal_nan=True)
    f32 = np.array([[0.95, 0.1, 0.3], [0.7, 0.2, 0.9]], np.float32)
    assert np.array_equal(conv(me, [f32], True, "residue"), f32.reshape(-1))
    assert np.array_equal(conv(me, [f32.astype(np.float64)], True, "residue"), f32.reshape(-1))     # float32 values in a float64 array
    bad = exact.copy()
    bad[1, 2] = 0.95                                             # the double 0.95 is no float32 value: float32 rounds it across the edge
    assert api.pp_char(np.float32(0.95)) == b"9" and orr.pp_char(np.float32(0.95)) == b"9"      # (the double itself gives "*")
    with pytest.raises(api.KalignAmdError, match=re.escape("family 0: residue confidence at (1, 2) is not a float32 value (0.95)")):
        conv(me, [bad], True, "residue")
    with pytest.raises(api.KalignAmdError, match="column confidence at \\(1,\\) is not a float32 value"):
        conv(me, [np.array([0.5, 0.1, 0.5])], False, "column")
    with pytest.raises(api.KalignAmdError, match="family 0: column confidences of shape \\(2,\\), not \\(3,\\)"):
        conv(me, [np.zeros(2, np.float32)], False, "column")
    assert conv(me, None, True, "residue") is None
