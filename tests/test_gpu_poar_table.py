"""GPU: the ensemble's POAR table as a file -- written from the members on the device (ka_ens_table_*), and read back into
a handle whose support comes from the table (ka_ens_open_table*; kalign_consensus_from_poar) -- against the stored cases
(tests/golden/poar_*.npz beside ens_*.npz), the reference's poar_table_write / kalign_consensus_from_poar when oracle/_ref
is built, and two independent device paths against each other at 256 x 300 x 8.  Byte identity throughout; the one
tolerance is the existing rel=1e-9 on the double score, whose integer sum is compared exactly beside it."""
import glob
import os
import sys

import numpy as np
import pytest

import poar_restate
from util import GOLDEN

pytestmark = pytest.mark.gpu

CASES = sorted(os.path.basename(f)[5:-4] for f in glob.glob(os.path.join(GOLDEN, "poar_*.npz")))
REAL = [c for c in CASES if c.startswith("real_")]
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


def _image(ctx, seqs, members):
    e = _ens(ctx, seqs, members)
    image = e.table_image()
    e.close()
    return image


def test_the_stored_cases_are_all_here():
    assert len(CASES) == 11 and len(REAL) == 6, CASES


# ---- write ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_write_stored_case(ctx, name, tmp_path):
    z, seqs, members, want = poar_restate.load_case(name)
    e = _ens(ctx, seqs, members)
    image = e.table_image()
    assert len(image) == int(want["size"]) and poar_restate.sha256(image) == str(want["sha256"])
    if "image" in want.files:
        assert image == want["image"].tobytes()
    assert e.table_size() == (int(want["size"]), int(want["n_entries"].sum()))
    assert e.stats()["table_entries"] == int(want["n_entries"].sum())
    p = str(tmp_path / "t.poar")
    e.write_table(p)
    assert open(p, "rb").read() == image
    e.close()


def _chunks_of_whole_rows(n_entries, n, cap):
    """chunks that hold entries when rows i are cut into chunks of at most cap entries (a longer row is a chunk of its own)"""
    rows, p = [], 0
    for i in range(n):
        rows.append(int(n_entries[p:p + n - 1 - i].sum()))
        p += n - 1 - i
    chunks, run = [], 0
    for t in rows:
        if run > 0 and run + t > cap:
            chunks.append(run)
            run = 0
        run += t
    chunks.append(run)
    return sum(1 for c in chunks if c)


@pytest.mark.parametrize("name", CASES)
def test_write_in_many_chunks(ctx, name, monkeypatch):
    """chunks of 7 entries: the table leaves the device in exactly as many chunks as whole rows allow, the same bytes.
    That is more than ten wherever the case has more than eleven sequences; three cases cannot reach ten, because a chunk
    is made of whole rows i and only rows with a pair hold entries: syn32 (10 sequences, 9 such rows) and
    real_bb11001_r3 / real_bb11001_r8 (4 sequences, 3 such rows)"""
    z, seqs, members, want = poar_restate.load_case(name)
    monkeypatch.setenv("KA_ENS_CHUNK", "7")
    e = _ens(ctx, seqs, members)
    image = e.table_image()
    chunks = e.stats()["table_chunks"]
    e.close()
    assert poar_restate.sha256(image) == str(want["sha256"]) and len(image) == int(want["size"])
    assert chunks == _chunks_of_whole_rows(want["n_entries"], len(seqs), 7)
    if len(seqs) > 11:
        assert chunks > 10


@pytest.mark.parametrize("name", CASES)
def test_letter_case_and_gap_byte_do_not_change_the_table(ctx, name):
    z, seqs, members, want = poar_restate.load_case(name)
    other = [[r.lower().replace("-", ".") for r in m] for m in members]
    assert poar_restate.sha256(_image(ctx, seqs, other)) == str(want["sha256"])


# ---- read -----------------------------------------------------------------------------------------------------------
def _check_table_stage(ctx, want, seqs, members, image):
    """what test_gpu_ensemble_stage._check_stage expects of the members, from a handle that only has the table"""
    t = ctx.ensemble_from_table([len(s) for s in seqs], image=image)
    m = _ens(ctx, seqs, members)
    assert t.n_runs == len(members)
    for k, rows in enumerate(members):
        s, v = t.score(rows)
        assert v == pytest.approx(float(want["scores"][k]), rel=1e-9, abs=1e-9), k
        assert s == m.score(rows)[0], k
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
    assert t.table_image() == image
    assert t.table_size() == (len(image), (len(image) - 16 - 2 * len(seqs) * (len(seqs) - 1)) // 8)
    t.close()
    m.close()


@pytest.mark.parametrize("name", CASES)
def test_read_device_written_table(ctx, name):
    z, seqs, members, want = poar_restate.load_case(name)
    _check_table_stage(ctx, z, seqs, members, _image(ctx, seqs, members))


@pytest.mark.parametrize("name", [c for c in CASES if "image" in np.load(os.path.join(GOLDEN, "poar_%s.npz" % c)).files])
def test_read_reference_written_table(ctx, name):
    z, seqs, members, want = poar_restate.load_case(name)
    _check_table_stage(ctx, z, seqs, members, want["image"].tobytes())


def test_reference_written_images_are_stored_for_seven_cases():
    assert sum("image" in np.load(os.path.join(GOLDEN, "poar_%s.npz" % c)).files for c in CASES) == 7


def test_read_in_many_chunks(ctx, monkeypatch):
    """the table-backed candidates and the table given back, in chunks of 7"""
    z, seqs, members, want = poar_restate.load_case("syn8")
    monkeypatch.setenv("KA_ENS_CHUNK", "7")
    t = ctx.ensemble_from_table([len(s) for s in seqs], image=want["image"].tobytes())
    for m in (1, 3):
        assert [x.decode() for x in t.consensus(seqs, m)] == [str(x) for x in z["cons%d" % m]]
        assert t.stats()["chunks"] > 10
    assert t.table_image() == want["image"].tobytes() and t.stats()["table_chunks"] > 10
    t.close()


@pytest.mark.parametrize("name", REAL)
def test_consensus_from_poar_and_save_poar_path(ctx, name, tmp_path):
    from kalign_amd import ensemble
    z, seqs, members, want = poar_restate.load_case(name)
    refined = [[str(r) for r in m] for m in z["refined"]]
    p = str(tmp_path / "saved.poar")
    plain = ensemble.finish_ensemble(ctx, members, seqs, rerun_refined=lambda k: refined[k])
    saved = ensemble.finish_ensemble(ctx, members, seqs, rerun_refined=lambda k: refined[k], save_poar_path=p)
    for key in ("rows", "scores", "best_k", "use_consensus", "consensus_score", "refined_score", "refined"):
        assert plain[key] == saved[key], key
    assert np.array_equal(plain["residue_confidence"], saved["residue_confidence"])
    assert np.array_equal(plain["column_confidence"], saved["column_confidence"])
    data = open(p, "rb").read()
    assert len(data) == int(want["size"]) and poar_restate.sha256(data) == str(want["sha256"])
    for m in z["min_supports"]:
        m = int(m)
        out = ensemble.consensus_from_poar(ctx, seqs, p, m)
        assert out["n_runs"] == len(members)
        assert [x.decode() for x in out["rows"]] == [str(x) for x in z["cons%d" % m]], m
        assert np.array_equal(out["residue_confidence"], z["cons%d_res_conf" % m]), m
        assert np.array_equal(out["column_confidence"], z["cons%d_col_conf" % m]), m
    from kalign_amd import KalignAmdError
    with pytest.raises(KalignAmdError, match="min_support"):
        ensemble.consensus_from_poar(ctx, seqs, p, 0)


# ---- live against the reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,n,length,runs", [(11, 64, 80, 8), (12, 128, 60, 5), (13, 40, 100, 16), (14, 48, 101, 6), (15, 24, 50, 32)])
def test_live_against_the_reference(ctx, seed, n, length, runs, tmp_path):
    """the device image == poar_table_write of the reference's table; the reference's kalign_consensus_from_poar on the
    DEVICE-written file == consensus_from_poar on the REFERENCE-written file"""
    import make_golden_ensemble as mg
    import make_golden_poar as mp
    from kalign_amd import ensemble
    if not mg.available():
        pytest.skip("oracle/_ref not built")
    seqs, members = mg.synthetic(n, length, runs, seed, moves=10)
    ref_image = mp.reference_image(members)
    e = _ens(ctx, seqs, members)
    dev = str(tmp_path / "device.poar")
    e.write_table(dev)
    e.close()
    assert open(dev, "rb").read() == ref_image
    ref = str(tmp_path / "reference.poar")
    open(ref, "wb").write(ref_image)
    for m in sorted({1, 2, ensemble.auto_min_support(runs), runs}):
        rows, res, col = mp.consensus_from_poar(seqs, dev, m)
        got = ensemble.consensus_from_poar(ctx, seqs, ref, m)
        assert [x.decode() for x in got["rows"]] == rows, m
        assert np.array_equal(got["residue_confidence"], res) and np.array_equal(got["column_confidence"], col), m


def test_live_bfs_queue_truncation_through_a_table(ctx):
    """the input of test_bfs_queue_truncation_against_the_reference through a table-backed handle: the same replay"""
    import make_golden_ensemble as mg
    if not mg.available():
        pytest.skip("oracle/_ref not built")
    seqs, members = mg.synthetic(128, 300, 8, 21, moves=8)
    want = mg.reference_stage(seqs, members, [3])
    t = ctx.ensemble_from_table([len(s) for s in seqs], image=_image(ctx, seqs, members))
    assert [x.decode() for x in t.consensus(seqs, 3)] == [str(x) for x in want["cons3"]]
    assert t.stats()["bfs_truncations"] > 0
    t.close()


# ---- member columns read where they lie ------------------------------------------------------------------------------
def test_table_with_member_columns_not_staged(ctx):
    """32 members x sequences of more than 468 residues: (3 + n_runs) x maxlen ints pass 64 KiB, so the table pass reads
    the members' columns from memory instead of LDS; the bytes of the restatement, and a handle opened from them agrees
    with the members on every score sum, on member 0's confidences and on the consensus"""
    import make_golden_ensemble as mg
    seqs, members = mg.synthetic(6, 520, 32, 31, moves=10)
    assert (3 + 32) * max(len(s) for s in seqs) * 4 > 65536
    m = _ens(ctx, seqs, members)
    image = m.table_image()
    assert image == poar_restate.poar_image(members)
    t = ctx.ensemble_from_table([len(s) for s in seqs], image=image)
    for rows in members:
        assert t.score(rows)[0] == m.score(rows)[0]
    rt, ct = t.confidence(members[0])
    rm, cm = m.confidence(members[0])
    assert np.array_equal(rt, rm) and np.array_equal(ct, cm)
    assert t.consensus(seqs, 11) == m.consensus(seqs, 11)
    t.close()
    m.close()


# ---- errors ---------------------------------------------------------------------------------------------------------
def test_errors(ctx, tmp_path):
    from kalign_amd import KalignAmdError, api
    z, seqs, members, want = poar_restate.load_case("syn3")
    lens = [len(s) for s in seqs]
    image = want["image"].tobytes()
    t = ctx.ensemble_from_table(lens, image=image)
    with pytest.raises(KalignAmdError, match="opened from a POAR table"):
        t.add_member(0, members[0])
    t.close()
    e = ctx.ensemble(lens, len(members))
    e.add_member(0, members[0])
    with pytest.raises(KalignAmdError, match="not added"):
        e.table_image()
    with pytest.raises(KalignAmdError, match="not added"):
        e.write_table(str(tmp_path / "never.poar"))
    assert not os.path.exists(str(tmp_path / "never.poar"))
    e.close()
    with pytest.raises(KalignAmdError, match="numseq 16 in the file, 15 sequences given"):
        ctx.ensemble_from_table(lens[:-1], image=image)
    short = list(lens)
    short[0] -= 1                                   # the last residue of sequence 0 is aligned with something
    with pytest.raises(KalignAmdError, match=r"residue ri = %d but sequence 0 has %d" % (short[0], short[0])):
        ctx.ensemble_from_table(short, image=image)
    with pytest.raises(KalignAmdError, match="truncated"):
        ctx.ensemble_from_table(lens, image=image[:-3])
    with pytest.raises(KalignAmdError, match="cannot open"):
        ctx.ensemble_from_table(lens, path=str(tmp_path / "missing.poar"))
    with pytest.raises(KalignAmdError, match="a path or an image"):
        ctx.ensemble_from_table(lens)
    with pytest.raises(KalignAmdError, match="0 bytes, shorter than the 16-byte header"):
        ctx.ensemble_from_table(lens, image=b"")
    with pytest.raises(KalignAmdError, match="n_runs members or a POAR table"):
        api.Ensemble(ctx, lens)


def test_closed_context():
    import kalign_amd
    from kalign_amd import KalignAmdError
    z, seqs, members, want = poar_restate.load_case("syn2")
    c = kalign_amd.Context(0)
    t = c.ensemble_from_table([len(s) for s in seqs], image=want["image"].tobytes())
    c.close()
    assert t.h is None
    with pytest.raises(KalignAmdError, match="closed"):
        c.ensemble_from_table([len(s) for s in seqs], image=want["image"].tobytes())


# ---- at size, device only -----------------------------------------------------------------------------------------------
def test_at_256x300x8(ctx):
    """two independent kernels count one set (entries by popcount / the candidates of consensus(seqs, 1) per level); a
    40-sequence subsample equals the numpy restatement; table-backed against member-backed on the full set"""
    import make_golden_ensemble as mg
    seqs, members = mg.synthetic(256, 300, 8, 7, moves=8)
    n = len(seqs)
    m = _ens(ctx, seqs, members)
    image = m.table_image()
    size, entries = m.table_size()
    assert size == len(image) == 16 + 4 * (n * (n - 1) // 2) + 8 * entries
    keys, masks = poar_restate.entries(image, n)
    assert len(keys) == entries
    pop = poar_restate.popcounts(masks)
    m.consensus(seqs, 1)
    level = m.stats()["level_candidates"]
    assert {L: int((pop == L).sum()) for L in range(1, 9) if (pop == L).any()} == level
    pick = np.sort(np.random.default_rng(3).choice(n, 40, replace=False))
    sub = [[mem[i] for i in pick] for mem in members]
    assert _image(ctx, [seqs[i] for i in pick], sub) == poar_restate.poar_image(sub)
    t = ctx.ensemble_from_table([len(s) for s in seqs], image=image)
    for rows in members:
        assert t.score(rows)[0] == m.score(rows)[0]
    rt, ct = t.confidence(members[0])
    rm, cm = m.confidence(members[0])
    assert np.array_equal(rt, rm) and np.array_equal(ct, cm)
    assert t.consensus(seqs, 3) == m.consensus(seqs, 3)
    t.close()
    m.close()
