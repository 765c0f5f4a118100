"""The host side of the codon stage (ka_cod_*): the names and the ABI revision; the table and the check -- the library's
host-only functions -- and the numpy restatement (tests/cod_restate.py) against every golden recorded from the reference
(tests/golden/cod_*.npz, tests/golden/make_codon_golden.py).  No GPU, no tolerance: every comparison is ==."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cod_restate as cr
from util import GOLDEN

NAMES = ("ka_cod_table", "ka_cod_fam_check", "ka_cod_fam_create", "ka_cod_fam_destroy", "ka_cod_fam_sequences", "ka_cod_fam_protein_size",
         "ka_cod_fam_protein", "ka_cod_fam_run", "ka_cod_fam_back", "ka_cod_fam_rows_size", "ka_cod_fam_rows", "ka_cod_fam_protein_rows_size",
         "ka_cod_fam_protein_rows", "ka_cod_fam_stats")
G = cr.goldens(GOLDEN)


def test_names_and_version():
    import kalign_amd
    from kalign_amd import api, codon
    L = kalign_amd.load_library()
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "kalign_amd.h")).read()
    declared = set(re.findall(r"\b(ka_[a-z_]+)\s*\(", hdr))
    for name in NAMES:
        assert name in declared and name in api.EXPORTS and hasattr(L, name), name
    assert L.ka_abi_version() >= 29
    for m in ("sequences", "proteins", "run", "back", "rows", "protein_rows", "stats"):
        assert callable(getattr(api.FamilyCodons, m)), m
    assert callable(api.Context.family_codons)
    for m in ("translate_families", "align_codon_families", "align_codons", "backtranslate_families", "mask_by_confidence"):
        assert callable(getattr(codon, m)), m
    assert kalign_amd.codon is codon
    assert api.COD_SEQ == cr.SEQ


def test_the_cases_are_there():
    assert {"table", "translate_all64", "translate_case", "translate_other_letters", "translate_stops", "back_rows", "e2e_fast",
            "e2e_default"} <= set(G)
    dna = [s for n in G if n.startswith("translate_") for s in G[n].texts("dna")]
    codons = {s[k:k + 3].upper() for s in dna for k in range(0, len(s), 3)}
    assert {c.encode() for c in cr.CODONS} <= codons
    for x in b"NUR":
        for place in range(3):
            assert any(c[place] == x for c in codons), (chr(x), place)
    assert any(s != s.upper() and s != s.lower() for s in dna)
    for n in ("e2e_fast", "e2e_default"):
        g = G[n]
        fams = g.families("dna")
        assert 3 <= len(fams) <= 4 and all(2 <= len(f) <= 16 and all(90 <= len(s) <= 600 for s in f) for f in fams)


def test_table_equals_the_reference():
    from kalign_amd import api
    t = api.codon_table()
    g = G["table"]
    assert g.texts("codons") == [c.encode() for c in cr.CODONS]
    assert t == b"".join(a if a else b"*" for a in g.texts("aa"))
    assert t == cr.table() == b"KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSS*CWCLFLF"
    assert [c for c, a in zip(cr.CODONS, t) if a == ord("*")] == ["TAA", "TAG", "TGA"]


def test_restatement_equals_every_translate_golden():
    n = 0
    for name, g in G.items():
        if not g.has("protein"):
            continue
        for s, p in zip(g.texts("dna"), g.texts("protein")):
            n += 1
            if p:
                r = cr.translate(s)
                assert r["protein"].encode() == p, (name, s)
                assert r["rec"][3] == len(s) // 3 and len(r["kept"]) == 3 * len(p) == 3 * (r["rec"][3] - r["rec"][4]), (name, s)
            else:                                            # (every codon a stop: the reference returns "", the stage refuses)
                with pytest.raises(ValueError, match="no protein"):
                    cr.translate(s)
    assert n > 150
    assert cr.translate(b"UUUUAAUAG")["protein"] == "XXX" and cr.translate(b"ATGGCNTAATGN")["rec"][3:] == [4, 1, 2]
    with pytest.raises(ValueError, match="4 residues, not a multiple of 3"):
        cr.translate(b"ATG-A")
    assert cr.translate(b"at g-GC.c\nTAA 12")["rec"] == [9, 2, 5, 3, 1, 0]


def test_restatement_equals_every_back_golden():
    g = G["back_rows"]
    rows = g.texts("rows")
    assert any(r.startswith(b"-") for r in rows) and any(r.endswith(b"-") for r in rows) and any(b"---" in r for r in rows)
    for s, row, want in zip(g.texts("dna"), rows, g.texts("codon_rows")):
        got = cr.backtranslate(row, s)
        assert got.encode() == want and len(got) == 3 * len(row), s
    for n in ("e2e_fast", "e2e_default"):
        g = G[n]
        for s, p, row, want in zip(g.texts("dna"), g.texts("protein"), g.texts("protein_rows"), g.texts("codon_rows")):
            assert row.replace(b"-", b"") == p
            assert cr.backtranslate(row, s).encode() == want
            assert want.replace(b"-", b"") == cr.translate(s)["kept"].encode()
    with pytest.raises(ValueError, match="the row holds 2 residues, the sequence 3 codons without stops"):
        cr.backtranslate("M-A", "ATGGCCTAAGCC")


def check(n_fam, fam_first, seq_off, n_bytes):
    import kalign_amd
    L = kalign_amd.load_library()
    f = np.ascontiguousarray(fam_first, np.int32)
    o = np.ascontiguousarray(seq_off, np.int64)
    rc = L.ka_cod_fam_check(n_fam, f.ctypes.data_as(C.c_void_p), o.ctypes.data_as(C.c_void_p), n_bytes)
    return rc, L.ka_last_error().decode()


def test_check_messages():
    assert check(2, [0, 2, 3], [0, 4, 4, 9], 9)[0] == 0                                      # (an empty sequence passes the check: create refuses it)
    assert check(2, [1, 2, 3], [0, 4, 4, 9], 9) == (1, "ka_cod_fam_check: fam_first does not ascend from 0 to numseq")
    assert check(2, [0, 2, 1], [0, 4, 4, 9], 9) == (1, "ka_cod_fam_check: fam_first does not ascend from 0 to numseq")
    assert check(2, [0, 2, 2], [0, 4, 4], 4) == (1, "ka_cod_fam_check: empty family")
    assert check(0, [0], [0], 0) == (1, "ka_cod_fam_check: bad arguments")
    assert check(1, [0, 2], [1, 4, 9], 9) == (1, "ka_cod_fam_check: seq_off does not ascend from 0 to n_bytes")
    assert check(1, [0, 2], [0, 10, 9], 9) == (1, "ka_cod_fam_check: seq_off does not ascend from 0 to n_bytes")
    assert check(1, [0, 2], [0, 4, 9], 10) == (1, "ka_cod_fam_check: seq_off does not ascend from 0 to n_bytes")
    assert check(2, [0, 1, 3], [0, 1, 3, 3 + 2 ** 31], 3 + 2 ** 31) == \
        (1, "ka_cod_fam_check: family 1, sequence 1: 2147483648 bytes; a sequence holds fewer than 2^31")
