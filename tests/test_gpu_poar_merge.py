"""GPU: new POAR tables from POAR tables -- ka_ens_merge (the union of two tables, the second's member bits shifted past the
first's) and ka_ens_select (a subset of the member bits in a new order, emptied entries dropped), Ensemble.merge / .select and
ensemble.extend_poar.  The oracle is the numpy restatement of the file from member rows (poar_restate.poar_image) and the stored
size / SHA-256 / image of tests/golden/poar_*.npz, which pin the reference's own file: the table of members 0..s-1 merged with
the table of members s..R-1 is the table of all R members, byte for byte.  Comparisons are == on bytes; the one tolerance is the
existing rel=1e-9 on the double score, whose integer sum is compared exactly beside it."""
import ctypes as C
import glob
import os
import sys

import numpy as np
import pytest

import poar_algebra
import poar_restate
from util import GOLDEN

pytestmark = pytest.mark.gpu

CASES = sorted(os.path.basename(f)[5:-4] for f in glob.glob(os.path.join(GOLDEN, "poar_*.npz")))
ALL_KINDS = ("syn8", "real_dna40_r8")                       # member / table operands on either side; elsewhere member x member
SPLITS = [(c, s) for c in CASES for s in poar_algebra.splits(np.load(os.path.join(GOLDEN, "ens_%s.npz" % c))["members"].shape[0])]
sys.path.insert(0, GOLDEN)


@pytest.fixture(scope="module")
def ctx():
    import kalign_amd
    c = kalign_amd.Context(0)
    yield c
    c.close()


def _ens(ctx, seqs, members):
    e = ctx.ensemble([len(s) for s in seqs], len(members))
    for k, rows in enumerate(members):
        e.add_member(k, rows)
    return e


def _operand(ctx, seqs, members, kind):
    """kind "m": a handle with these members; "t": a handle opened from their table"""
    e = _ens(ctx, seqs, members)
    if kind == "m":
        return e
    t = ctx.ensemble_from_table([len(s) for s in seqs], image=e.table_image())
    e.close()
    return t


def _merged_image(ctx, seqs, a_rows, b_rows, kinds="mm"):
    """image of merge(A, B), both operands unchanged by it"""
    from kalign_amd import api
    a, b = _operand(ctx, seqs, a_rows, kinds[0]), _operand(ctx, seqs, b_rows, kinds[1])
    before = a.table_image(), b.table_image()
    m = a.merge(b)
    image = m.table_image()
    assert m.n_runs == len(a_rows) + len(b_rows)
    assert api.check_table(image, [len(s) for s in seqs]) == (m.n_runs, m.table_size()[1])
    assert (a.table_image(), b.table_image()) == before
    for e in (m, a, b):
        e.close()
    return image


def _selected_image(ctx, seqs, members, sel, kind="m"):
    from kalign_amd import api
    e = _operand(ctx, seqs, members, kind)
    s = e.select(sel)
    image = s.table_image()
    assert s.n_runs == len(sel)
    assert api.check_table(image, [len(s) for s in seqs]) == (len(sel), s.table_size()[1])
    s.close()
    e.close()
    return image


def test_the_stored_cases_are_all_here():
    assert len(CASES) == 11 and len(SPLITS) == 27 and ("syn32", 16) in SPLITS and ("syn32", 31) in SPLITS


# ---- 1. split and merge equals the whole -------------------------------------------------------------------------------
@pytest.mark.parametrize("name,s", SPLITS)
def test_split_and_merge_equals_the_whole(ctx, name, s):
    z, seqs, members, want = poar_restate.load_case(name)
    for kinds in (("mm", "mt", "tm", "tt") if name in ALL_KINDS else ("mm",)):
        image = _merged_image(ctx, seqs, members[:s], members[s:], kinds)
        assert len(image) == int(want["size"]) and poar_restate.sha256(image) == str(want["sha256"]), kinds
        if "image" in want.files:
            assert image == want["image"].tobytes(), kinds


# ---- 2. the reference's own bytes ---------------------------------------------------------------------------------------
def _r3_image(ctx, case):
    z3, seqs, m3, w3 = poar_restate.load_case(case + "_r3")
    if "image" in w3.files:
        return w3["image"].tobytes()
    e = _ens(ctx, seqs, m3)
    image = e.table_image()
    e.close()
    assert poar_restate.sha256(image) == str(w3["sha256"])
    return image


@pytest.mark.parametrize("case", ["real_bb11001", "real_bb30014", "real_dna40"])
def test_saved_r3_table_and_five_new_members_give_the_r8_file(ctx, case):
    z8, seqs, m8, w8 = poar_restate.load_case(case + "_r8")
    old = ctx.ensemble_from_table([len(s) for s in seqs], image=_r3_image(ctx, case))
    new = _ens(ctx, seqs, m8[3:])
    merged = old.merge(new)
    image = merged.table_image()
    assert merged.n_runs == 8
    assert len(image) == int(w8["size"]) and poar_restate.sha256(image) == str(w8["sha256"])
    if "image" in w8.files:
        assert image == w8["image"].tobytes()
    for e in (merged, new, old):
        e.close()


@pytest.mark.parametrize("case", ["real_bb11001", "real_bb30014", "real_dna40"])
def test_extend_poar(ctx, case, tmp_path):
    from kalign_amd import ensemble
    z8, seqs, m8, w8 = poar_restate.load_case(case + "_r8")
    p3, p8 = str(tmp_path / "r3.poar"), str(tmp_path / "r8.poar")
    with open(p3, "wb") as f:
        f.write(_r3_image(ctx, case))
    for ms in z8["min_supports"]:
        ms = int(ms)
        if os.path.exists(p8):
            os.remove(p8)
        out = ensemble.extend_poar(ctx, seqs, p3, m8[3:], save_poar_path=p8, min_support=ms)
        data = open(p8, "rb").read()
        assert len(data) == int(w8["size"]) and poar_restate.sha256(data) == str(w8["sha256"]), ms
        assert (out["n_runs"], out["n_old"]) == (8, 3)
        assert out["scores"] == pytest.approx([float(x) for x in z8["scores"][3:]], rel=1e-9, abs=1e-9)
        assert [x.decode() for x in out["rows"]] == [str(x) for x in z8["cons%d" % ms]], ms
        assert np.array_equal(out["residue_confidence"], z8["cons%d_res_conf" % ms]), ms
        assert np.array_equal(out["column_confidence"], z8["cons%d_col_conf" % ms]), ms
    # no threshold given: kalign_ensemble's automatic one for the 8 members of the merged table, nothing written
    assert ensemble.auto_min_support(8) == 3 and 3 in z8["min_supports"]
    out = ensemble.extend_poar(ctx, seqs, p3, m8[3:])
    assert [x.decode() for x in out["rows"]] == [str(x) for x in z8["cons3"]]
    assert sorted(os.listdir(str(tmp_path))) == ["r3.poar", "r8.poar"]


# ---- 3. the result behaves as the whole ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["syn8", "syn8dna", "real_bb30014_r8"])
def test_merged_handle_behaves_as_the_whole(ctx, name, monkeypatch):
    """what test_gpu_poar_table expects of a handle opened from the members' table, of the merged handle"""
    want, seqs, members, stored = poar_restate.load_case(name)
    s = len(members) // 2
    a, b, m = _ens(ctx, seqs, members[:s]), _ens(ctx, seqs, members[s:]), _ens(ctx, seqs, members)
    t = a.merge(b)
    assert t.n_runs == len(members)
    for k, rows in enumerate(members):
        sm, v = t.score(rows)
        assert v == pytest.approx(float(want["scores"][k]), rel=1e-9, abs=1e-9), k
        assert sm == m.score(rows)[0], k
    r, c = t.confidence(members[0])
    assert np.array_equal(r, want["m0_res_conf"]) and np.array_equal(c, want["m0_col_conf"])
    for ms in want["min_supports"]:
        ms = int(ms)
        rows = [x.decode() for x in t.consensus(seqs, ms)]
        assert rows == [str(x) for x in want["cons%d" % ms]], ms
        assert t.score(rows)[1] == pytest.approx(float(want["cons%d_score" % ms]), rel=1e-9, abs=1e-9), ms
        assert t.score(rows)[0] == m.score(rows)[0], ms
        r, c = t.confidence(rows)
        assert np.array_equal(r, want["cons%d_res_conf" % ms]), ms
        assert np.array_equal(c, want["cons%d_col_conf" % ms]), ms
    image = t.table_image()
    assert len(image) == int(stored["size"]) and poar_restate.sha256(image) == str(stored["sha256"])
    entries = (len(image) - 16 - 2 * len(seqs) * (len(seqs) - 1)) // 8
    assert t.table_size() == (len(image), entries)
    monkeypatch.setenv("KA_ENS_CHUNK", "7")                  # read when a handle is made: the next result hands its table over in chunks of 7
    t7 = a.merge(b)
    st = t7.stats()
    assert st["table_entries"] == entries and st["table_count_ms"] > 0 and st["table_write_ms"] > 0
    assert t7.table_image() == image and t7.stats()["table_chunks"] > 10
    for e in (t7, t, m, b, a):
        e.close()


# ---- 4. order, 5. chain ---------------------------------------------------------------------------------------------------
def test_order_matters(ctx):
    z, seqs, members, want = poar_restate.load_case("syn3")
    ab = _merged_image(ctx, seqs, members[:1], members[1:])
    ba = _merged_image(ctx, seqs, members[1:], members[:1])
    assert ba == poar_restate.poar_image(members[1:] + members[:1])
    assert ab == want["image"].tobytes() and ab != ba


def test_chain_one_member_at_a_time(ctx):
    z, seqs, members, want = poar_restate.load_case("syn8")
    t = _ens(ctx, seqs, members[:1])
    for k in range(1, 8):
        one = _ens(ctx, seqs, members[k:k + 1])
        nxt = t.merge(one)
        one.close()
        t.close()
        t = nxt
    assert t.n_runs == 8 and t.table_image() == want["image"].tobytes()
    t.close()


# ---- 6. the smallest shapes that can break the kernel: one member against one member, the restatement is the oracle -------
def _letters(n, k):
    return "".join("ACDEFGHIKLMNPQRSTVWY"[(7 * k + 3 * p) % 20] for p in range(n))


def _packed(seqs, shifted=()):
    """all rows left-packed, the rows in `shifted` one column to the right"""
    w = max(len(s) for s in seqs) + 1
    return [("-" + s if k in shifted else s).ljust(w, "-") for k, s in enumerate(seqs)]


def test_pair_lists_around_one_tile_and_past_two(ctx):
    """lengths 63 / 64 / 65 / 129 / 130, member B with the odd rows one column to the right: lists of 62 to 65 entries on
    either side with 0, 63 or 64 shared keys, and lists of 129 / 128 entries (past two tiles of 64)"""
    seqs = [_letters(n, k) for k, n in enumerate((63, 64, 65, 129, 130))]
    a, b = _packed(seqs), _packed(seqs, shifted=(1, 3))
    ia, ib = (poar_restate.pair_counts(poar_restate.poar_image([x]), 5).tolist() for x in (a, b))
    both = poar_restate.pair_counts(poar_restate.poar_image([a, b]), 5).tolist()
    shared = [x + y - u for x, y, u in zip(ia, ib, both)]
    assert {62, 63, 64, 65} <= set(ia + ib) and {0, 63, 64} <= set(shared) and max(ia) == 129
    assert _merged_image(ctx, seqs, [a], [b]) == poar_restate.poar_image([a, b])
    assert _merged_image(ctx, seqs, [b], [a], "tt") == poar_restate.poar_image([b, a])


def test_equal_operands_share_every_key(ctx):
    seqs = [_letters(n, k) for k, n in enumerate((63, 64, 65, 129, 130))]
    a = _packed(seqs)
    image = _merged_image(ctx, seqs, [a], [a])
    assert image == poar_restate.poar_image([a, a])
    assert set(poar_restate.entries(image, 5)[1].tolist()) == {3}


def test_a_pair_without_entries(ctx):
    seqs = ["AC", "GT"]
    none, full = ["AC--", "--GT"], ["AC", "GT"]
    for x, y in ((none, full), (full, none), (none, none)):
        for kinds in ("mm", "tt"):
            assert _merged_image(ctx, seqs, [x], [y], kinds) == poar_restate.poar_image([x, y])
    assert len(poar_restate.poar_image([none, none])) == 20


def test_residue_4095_in_the_key(ctx):
    seqs = [_letters(4096, 0), _letters(4096, 1)]
    a, b = _packed(seqs), _packed(seqs, shifted=(1,))
    image = _merged_image(ctx, seqs, [a], [b])
    assert image == poar_restate.poar_image([a, b])
    assert int(poar_restate.entries(image, 2)[0].max()) == 4095 << 20 | 4095


def test_members_whose_columns_do_not_fit_lds(ctx):
    """the input of test_table_with_member_columns_not_staged: 32 members selected down to 16 + 16 and merged back"""
    import make_golden_ensemble as mg
    seqs, members = mg.synthetic(6, 520, 32, 31, moves=10)
    assert (3 + 32) * max(len(s) for s in seqs) * 4 > 65536
    m = _ens(ctx, seqs, members)
    lo, hi = m.select(range(16)), m.select(range(16, 32))
    back = lo.merge(hi)
    whole = poar_restate.poar_image(members)
    assert m.table_image() == whole and back.table_image() == whole
    assert lo.table_image() == poar_restate.poar_image(members[:16])
    for e in (back, hi, lo, m):
        e.close()


# ---- 7. select ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sel", [[k] for k in range(8)] + [list(range(1, 8)), list(range(7, -1, -1))], ids=str)
def test_select_on_syn8(ctx, sel):
    z, seqs, members, want = poar_restate.load_case("syn8")
    for kind in "mt":
        assert _selected_image(ctx, seqs, members, sel, kind) == poar_restate.poar_image([members[k] for k in sel]), kind


def test_select_identity(ctx):
    z, seqs, members, want = poar_restate.load_case("syn8")
    for kind in "mt":
        assert _selected_image(ctx, seqs, members, range(8), kind) == want["image"].tobytes()


def test_select_bit_31(ctx):
    z, seqs, members, want = poar_restate.load_case("syn32")
    assert _selected_image(ctx, seqs, members, [31, 0], "t") == poar_restate.poar_image([members[31], members[0]])
    assert _selected_image(ctx, seqs, members, [31, 0], "m") == poar_restate.poar_image([members[31], members[0]])


@pytest.mark.parametrize("s", [1, 4, 7])
def test_select_both_halves_and_merge_back(ctx, s):
    z, seqs, members, want = poar_restate.load_case("syn8dna")
    t = ctx.ensemble_from_table([len(x) for x in seqs], image=want["image"].tobytes())
    lo, hi = t.select(range(s)), t.select(range(s, 8))
    back = lo.merge(hi)
    assert back.table_image() == want["image"].tobytes() == t.table_image()
    for e in (back, hi, lo, t):
        e.close()


def test_select_can_empty_a_pair(ctx):
    from kalign_amd import api
    seqs = ["AC", "GT"]
    none, full = ["AC--", "--GT"], ["AC", "GT"]
    a, b = _ens(ctx, seqs, [none]), _ens(ctx, seqs, [full])
    m = a.merge(b)
    first = m.select([0])
    image = first.table_image()
    assert image == poar_restate.poar_image([none]) and len(image) == 20
    assert api.check_table(image, [2, 2]) == (1, 0)
    assert m.select([1]).table_image() == poar_restate.poar_image([full])
    for e in (first, m, b, a):
        e.close()


# ---- 8. at size, device against device ------------------------------------------------------------------------------------
def test_at_256x300x8(ctx):
    import make_golden_ensemble as mg
    seqs, members = mg.synthetic(256, 300, 8, 7, moves=8)
    whole, lo, hi = _ens(ctx, seqs, members), _ens(ctx, seqs, members[:4]), _ens(ctx, seqs, members[4:])
    image = whole.table_image()
    merged = lo.merge(hi)
    assert merged.table_image() == image
    first = whole.select(range(4))
    assert first.table_image() == lo.table_image()
    assert merged.consensus(seqs, 3) == whole.consensus(seqs, 3)
    for e in (first, merged, hi, lo, whole):
        e.close()


# ---- 9. errors ------------------------------------------------------------------------------------------------------------
def test_errors(ctx):
    import kalign_amd
    from kalign_amd import KalignAmdError
    z, seqs, members, want = poar_restate.load_case("syn3")
    lens = [len(s) for s in seqs]
    image = want["image"].tobytes()
    t = ctx.ensemble_from_table(lens, image=image)
    m = _ens(ctx, seqs, members)

    def fails(pattern, call):
        with pytest.raises(KalignAmdError, match=pattern):
            call()
        assert t.table_image() == image and m.table_image() == image

    closed = _ens(ctx, seqs, members[:1])
    closed.close()
    fails("NULL handle", lambda: t.merge(closed))
    fails("NULL handle", lambda: closed.merge(m))
    fails("NULL handle", lambda: closed.select([0]))
    other = kalign_amd.Context(0)
    elsewhere = other.ensemble_from_table(lens, image=image)
    fails("different contexts", lambda: t.merge(elsewhere))
    fails("different contexts", lambda: elsewhere.merge(m))
    assert elsewhere.table_image() == image
    other.close()
    fewer = ctx.ensemble(lens[:-1], 1)
    fails("numseq 16 in the first handle, 15 in the second", lambda: t.merge(fewer))
    fails("numseq 15 in the first handle, 16 in the second", lambda: fewer.merge(m))
    longer = list(lens)
    longer[5] += 1
    longer[9] += 1
    uneven = ctx.ensemble(longer, 1)
    fails("sequence 5 has %d residues in the first handle, %d in the second" % (lens[5], lens[5] + 1), lambda: m.merge(uneven))
    thirty = ctx.ensemble(lens, 30)
    fails(r"3 \+ 30 members exceed 32", lambda: t.merge(thirty))
    fails(r"30 \+ 3 members exceed 32", lambda: thirty.merge(m))
    partial = ctx.ensemble(lens, 3)
    partial.add_member(0, members[0])
    partial.add_member(2, members[2])
    fails("member 1 not added", lambda: t.merge(partial))
    fails("member 1 not added", lambda: partial.merge(m))
    fails("member 1 not added", lambda: partial.select([0]))
    for e in (t, m):
        fails(r"n = 0 outside 1\.\.3", lambda: e.select([]))
        fails(r"n = 4 outside 1\.\.3", lambda: e.select([0, 1, 2, 0]))
        fails("member index 3 out of range", lambda: e.select([0, 3]))
        fails("member index -1 out of range", lambda: e.select([-1]))
        fails("member 1 given twice", lambda: e.select([1, 1]))
    # *out is untouched by a failing call
    h = C.c_void_p(12345)
    assert ctx.L.ka_ens_merge(t.h, thirty.h, C.byref(h)) != 0 and h.value == 12345
    none = np.zeros(1, np.int32)
    assert ctx.L.ka_ens_select(t.h, none.ctypes.data_as(C.c_void_p), 0, C.byref(h)) != 0 and h.value == 12345
    assert ctx.L.ka_ens_merge(t.h, m.h, None) != 0 and b"NULL" in ctx.L.ka_last_error()
    # a result takes no members, like any table-backed handle
    merged, picked = t.merge(m), m.select([2])
    for e in (merged, picked):
        with pytest.raises(KalignAmdError, match="opened from a POAR table"):
            e.add_member(0, members[0])
    assert merged.n_runs == 6 and picked.n_runs == 1
    for e in (picked, merged, partial, thirty, uneven, fewer, m, t):
        e.close()


def test_closed_context():
    import kalign_amd
    z, seqs, members, want = poar_restate.load_case("syn2")
    c = kalign_amd.Context(0)
    a, b = _ens(c, seqs, members[:1]), _ens(c, seqs, members[1:])
    merged = a.merge(b)
    picked = merged.select([1])
    c.close()
    assert merged.h is None and picked.h is None and a.h is None
