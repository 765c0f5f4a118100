"""The host side of the input stage (ka_in_*): the names and the ABI revision; the three tables, detection and the order
-- the library's host-only functions -- and the numpy restatement (tests/in_restate.py) against every golden recorded
from the reference (tests/golden/in_*.npz, tests/golden/make_input_golden.py); the check's messages; pfasum_auto.  No GPU,
no tolerance: every comparison is ==."""
import ctypes as C
import re

import numpy as np
import pytest

import in_restate as ir
from util import GOLDEN

NAMES = ("ka_in_tables", "ka_in_detect", "ka_in_order", "ka_in_fam_check", "ka_in_fam_create", "ka_in_fam_destroy", "ka_in_fam_sequences",
         "ka_in_fam_families", "ka_in_fam_order", "ka_in_fam_size", "ka_in_fam_encoded", "ka_in_fam_run", "ka_in_fam_rows_size", "ka_in_fam_rows",
         "ka_in_fam_stats")
G = ir.goldens(GOLDEN)
# the letters no alphabet of the reference names (alphabet.c:179-302): they are written as code 0 and counted
NO_CODE = {1: "EFIJLOPQXZ", 0: "JO"}


def by_name(name):
    return next(g for g in G if g.name == name)


def test_names_and_version():
    import os
    import kalign_amd
    from kalign_amd import api, prepare
    L = kalign_amd.load_library()
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "kalign_amd.h")).read()
    declared = set(re.findall(r"\b(ka_[a-z_]+)\s*\(", hdr))
    for name in NAMES:
        assert name in declared and name in api.EXPORTS and hasattr(L, name), name
    assert L.ka_abi_version() >= 28
    for m in ("sequences", "families", "order", "encoded", "run", "rows", "stats"):
        assert callable(getattr(api.FamilyInput, m)), m
    assert callable(api.Context.family_input)
    for m in ("prepare_families", "align_families", "align", "pfasum_auto"):
        assert callable(getattr(prepare, m)), m
    assert kalign_amd.prepare is prepare
    assert api.IN_SEQ == ir.SEQ and api.IN_FAM == ir.FAM


def test_the_cases_are_there():
    names = {g.name for g in G}
    assert {"table_protein", "table_dna", "edge8", "edge9", "equal_named", "equal_unnamed", "status_unaligned", "status_aligned",
            "status_unknown_gaps", "status_unknown_same", "e2e_protein_fast", "e2e_protein_default", "e2e_dna_fast", "e2e_dna_default",
            "file_route"} <= names
    for k, want in (("table_protein", 0), ("table_dna", 1)):
        g = by_name(k)
        letters = set(b"".join(g.seqs))
        assert set(range(65, 91)) | set(range(97, 123)) <= letters and int(g.biotype) == want
    assert {int(by_name(k).status) for k in names if k.startswith("status_")} == {1, 2, 3}
    for g in G:
        if g.has("rows"):
            assert len(g.seqs) <= 24 and g.rows.shape[0] == len(g.seqs) and max(ir.scan(s)["residues"] for s in g.seqs) <= 120


def letter_pairs(g):
    """(letter, tree code, alignment code) of every residue of a golden recorded through the library entry"""
    res = ir.family(g.seqs, biotype=int(g.biotype))
    letters = np.concatenate(res["letters"])
    assert np.array_equal([len(x) for x in res["letters"]], g.lens)
    return letters, g.tree_codes, g.codes


def test_tables_equal_the_reference():
    from kalign_amd import api
    T = api.input_tables()
    assert T.shape == (3, 128) and T.dtype == np.int8 and np.array_equal(T, ir.tables())
    letter = np.array([chr(b).isalpha() for b in range(128)])
    assert (T[:, ~letter] == -1).all()
    assert np.array_equal(T[:, 65:91], T[:, 97:123])
    seen = {0: set(), 1: set()}
    for g in G:
        if not g.has("tree_codes"):
            continue
        bt = int(g.biotype)
        letters, tree, aln = letter_pairs(g)
        t_tree, t_aln = (T[0], T[0]) if bt == 1 else (T[1], T[2])
        for t, want in ((t_tree, tree), (t_aln, aln)):
            got = t[letters]
            # a letter without a code: the reference stores 0 (convert_msa_to_internal)
            assert np.array_equal(np.where(got < 0, 0, got), want), g.name
        seen[bt] |= set(letters.tolist())
    for bt, t in ((1, T[0]), (0, T[1]), (0, T[2])):
        assert seen[bt] >= set(range(65, 91)) | set(range(97, 123))          # the goldens pin every letter's code
        assert "".join(chr(b) for b in range(65, 91) if t[b] < 0) == NO_CODE[bt]


def test_detect_on_the_goldens():
    from kalign_amd import api
    n = 0
    for g in G:
        if not g.has("biotype"):
            continue
        freq = ir.histogram(g.seqs)
        assert api.input_detect(freq) == int(g.biotype) == ir.detect(freq), g.name
        n += 1
    assert n >= 10
    assert int(by_name("edge8").biotype) == 0 and int(by_name("edge9").biotype) == 1     # (what the reference said when they were recorded)
    with pytest.raises(api.KalignAmdError, match="ka_in_detect: could not determine the alphabet"):
        api.input_detect(np.zeros(128, np.int64))                                          # 0.0 == 0.0: the one tie known
    assert ir.detect(np.zeros(128, np.int64)) is None


def test_order_on_the_goldens():
    from kalign_amd import api
    n = 0
    for g in G:
        if not g.has("ranks"):
            continue
        res = np.array([ir.scan(s)["residues"] for s in g.seqs], np.int32)
        got = api.input_order([len(res)], res)
        assert np.array_equal(got, g.ranks) and np.array_equal(ir.order(res), g.ranks), g.name
        assert np.array_equal(res[got], g.lens)
        # the names the reference's library entry makes up give the same order
        assert np.array_equal(api.input_order([len(res)], res, ["s%07d" % i for i in range(len(res))]), g.ranks)
        n += 1
    assert n >= 9
    g = by_name("equal_unnamed")                                                         # one length, no names: input order
    assert len(set(g.lens.tolist())) == 1 and g.ranks.tolist() == list(range(len(g.seqs)))


def test_order_by_name_and_in_batches():
    from kalign_amd import api
    g = by_name("equal_named")
    res = np.array([ir.scan(s)["residues"] for s in g.seqs], np.int32)
    assert len(set(res.tolist())) == 1
    got = api.input_order([len(res)], res, g.names)
    assert [g.names[i] for i in got] == sorted(g.names) and got.tolist() != sorted(got.tolist())
    assert np.array_equal(got, ir.order(res, g.names))
    # equal names fall back on the input index; a prefix sorts first; bytes compare unsigned; only 256 bytes count
    long_a, long_b = b"x" * 256 + b"b", b"x" * 256 + b"a"
    names = [b"b", b"ab", b"a", b"a", b"\xe9", b"", long_a, long_b]
    res = np.full(len(names), 7, np.int32)
    got = api.input_order([len(names)], res, names)
    assert got.tolist() == [5, 2, 3, 1, 0, 6, 7, 4] and np.array_equal(got, ir.order(res, names))
    # several families: each sorts inside its own range
    sizes, rng = [1, 3, 2, 5], np.random.default_rng(5)
    res = rng.integers(1, 4, sum(sizes)).astype(np.int32)
    got = api.input_order(sizes, res)
    o = 0
    for n in sizes:
        assert np.array_equal(got[o:o + n], o + ir.order(res[o:o + n]))
        o += n


def test_restatement_equals_every_golden():
    for g in G:
        bt = int(g.biotype) if g.has("biotype") else -1
        r = ir.family(g.seqs, g.names, bt)
        if g.has("biotype"):
            assert ir.detect(r["freq"]) == bt, g.name
        if g.has("status"):
            assert r["fam"]["aligned"] == int(g.status), g.name
        if g.has("ranks"):
            assert np.array_equal(r["order"], g.ranks) and np.array_equal(r["seqs"][r["order"], 0], g.lens), g.name
            for mine, ref in ((r["tree_codes"], g.tree_codes), (r["codes"], g.codes)):
                assert np.array_equal(np.concatenate(mine), ref), g.name
        if g.has("rows"):
            # the rows hold the residues as given, in input order
            for s, row in zip(g.seqs, g.row_bytes()):
                assert bytes(c for c in row if chr(c).isalpha()) == ir.scan(s)["letters"].tobytes(), g.name
        assert r["freq"].sum() == sum(len(s) for s in g.seqs)


def test_checksum_and_rule_by_hand():
    # GCGchecksum by its definition on a sequence longer than one cycle of the 57 weights
    s = b"aCdEfGhIkLmNpQrStVwY" * 4
    want = 0
    for i, c in enumerate(s.upper()):
        want = (want + (i % 57 + 1) * c) % 10000
    assert ir.scan(s)["checksum"] == want
    r = ir.scan(b"A-c.\t1 Z*\n~\x7f[")
    assert (r["letters"].tobytes(), r["gap_characters"], r["dropped"], r["bad"]) == (b"AcZ", 5, 5, -1)
    assert ir.scan(b"AC\xc3\xa9G\xff")["bad"] == 2


def check(n_fam, fam_first, seq_off, n_bytes):
    import kalign_amd
    L = kalign_amd.load_library()
    f = np.ascontiguousarray(fam_first, np.int32)
    o = np.ascontiguousarray(seq_off, np.int64)
    rc = L.ka_in_fam_check(n_fam, f.ctypes.data_as(C.c_void_p), o.ctypes.data_as(C.c_void_p), n_bytes)
    return rc, L.ka_last_error().decode()


def test_check_messages():
    assert check(2, [0, 2, 3], [0, 4, 4, 9], 9)[0] == 0                                      # (an empty sequence passes the check: create refuses it)
    assert check(2, [1, 2, 3], [0, 4, 4, 9], 9) == (1, "ka_in_fam_check: fam_first does not ascend from 0 to numseq")
    assert check(2, [0, 2, 1], [0, 4, 4, 9], 9) == (1, "ka_in_fam_check: fam_first does not ascend from 0 to numseq")
    assert check(2, [0, 2, 2], [0, 4, 4], 4) == (1, "ka_in_fam_check: empty family")
    assert check(0, [0], [0], 0) == (1, "ka_in_fam_check: bad arguments")
    assert check(1, [0, 2], [1, 4, 9], 9) == (1, "ka_in_fam_check: seq_off does not ascend from 0 to n_bytes")
    assert check(1, [0, 2], [0, 10, 9], 9) == (1, "ka_in_fam_check: seq_off does not ascend from 0 to n_bytes")
    assert check(1, [0, 2], [0, 4, 9], 10) == (1, "ka_in_fam_check: seq_off does not ascend from 0 to n_bytes")
    assert check(2, [0, 1, 3], [0, 1, 3, 3 + 2 ** 31], 3 + 2 ** 31) == \
        (1, "ka_in_fam_check: family 1, sequence 1: 2147483648 bytes; a sequence holds fewer than 2^31")


def test_pfasum_auto():
    from kalign_amd.prepare import pfasum_auto
    assert pfasum_auto(100, 149) == "PFASUM43" and pfasum_auto(100, 150) == "PFASUM60"
    assert pfasum_auto(2, 3) == "PFASUM60" and pfasum_auto(200, 299) == "PFASUM43" and pfasum_auto(200, 300) == "PFASUM60"
    assert pfasum_auto(0, 10) == "PFASUM43" and pfasum_auto(7, 7) == "PFASUM43"
