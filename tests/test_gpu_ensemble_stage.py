"""GPU: the ensemble consensus stage (ka_ens: scores, consensus alignment, confidences) against the reference's
POAR-table code (lib/src/poar.c, consensus_msa.c) -- stored cases (tests/golden/ens_*.npz, make_golden_ensemble.py),
live randomized cases when oracle/_ref is built, kalign_ensemble's decisions (kalign_amd.ensemble), error paths and a
property run at 2048 x 300 x 8."""
import ctypes as C
import glob
import os
import sys

import numpy as np
import pytest

from util import GOLDEN

pytestmark = pytest.mark.gpu

CASES = sorted(os.path.basename(f)[4:-4] for f in glob.glob(os.path.join(GOLDEN, "ens_*.npz")))
REAL = [c for c in CASES if c.startswith("real_")]
sys.path.insert(0, GOLDEN)


@pytest.fixture(scope="module")
def ctx():
    import kalign_amd
    c = kalign_amd.Context(0)
    yield c
    c.close()


def _load(name):
    z = np.load(os.path.join(GOLDEN, "ens_%s.npz" % name))
    seqs = [str(s) for s in z["seqs"]]
    members = [["".join(r) for r in m] for m in z["members"]]
    return z, seqs, members


def _ens(ctx, seqs, members):
    e = ctx.ensemble([len(s) for s in seqs], len(members))
    for k, rows in enumerate(members):
        e.add_member(k, rows)
    return e


def _check_stage(ctx, want, seqs, members):
    e = _ens(ctx, seqs, members)
    for k, rows in enumerate(members):
        assert e.score(rows)[1] == pytest.approx(float(want["scores"][k]), rel=1e-9, abs=1e-9), k
    r, c = e.confidence(members[0])
    assert np.array_equal(r, want["m0_res_conf"]) and np.array_equal(c, want["m0_col_conf"])
    for m in want["min_supports"]:
        m = int(m)
        rows = [x.decode() for x in e.consensus(seqs, m)]
        assert rows == [str(x) for x in want["cons%d" % m]], m
        assert e.score(rows)[1] == pytest.approx(float(want["cons%d_score" % m]), rel=1e-9, abs=1e-9), m
        r, c = e.confidence(rows)
        assert np.array_equal(r, want["cons%d_res_conf" % m]), m
        assert np.array_equal(c, want["cons%d_col_conf" % m]), m
    e.close()


def test_golden_cases_exist():
    assert len(CASES) >= 5, CASES


@pytest.mark.parametrize("name", CASES)
def test_stage_against_golden(ctx, name):
    z, seqs, members = _load(name)
    _check_stage(ctx, z, seqs, members)


def test_real_member_cases_exist():
    assert len(REAL) >= 6, REAL


@pytest.mark.parametrize("name", REAL)
def test_finish_ensemble_equals_kalign_ensemble(ctx, name):
    """members of the reference's own ensemble loop (kalign_run_seeded), its refined re-runs and kalign_ensemble's output:
    finish_ensemble chooses the same rows (selection / consensus / refinement) with the same confidences"""
    from kalign_amd import ensemble
    z, seqs, members = _load(name)
    refined = [[str(r) for r in m] for m in z["refined"]]
    out = ensemble.finish_ensemble(ctx, members, seqs, rerun_refined=lambda k: refined[k])
    assert [x.decode() for x in out["rows"]] == [str(x) for x in z["ens_rows"]]
    assert np.array_equal(out["residue_confidence"], z["ens_res_conf"])
    assert np.array_equal(out["column_confidence"], z["ens_col_conf"])
    # an explicit threshold: the consensus, no selection
    m = int(z["min_supports"][0])
    out = ensemble.finish_ensemble(ctx, members, seqs, min_support=m)
    assert out["use_consensus"] and [x.decode() for x in out["rows"]] == [str(x) for x in z["cons%d" % m]]


def test_refined_member_replaces_the_winner_only_when_better(ctx):
    from kalign_amd import ensemble
    z, seqs, members = _load("real_bb30014_r8")                # kalign_ensemble kept the selection here
    scores = [float(s) for s in z["scores"]]
    best = ensemble.select(scores)
    asked = []

    def rerun(k):
        asked.append(k)
        return members[k]                      # the same rows: not better, kept out
    out = ensemble.finish_ensemble(ctx, members, seqs, rerun_refined=rerun)
    if out["use_consensus"]:
        assert asked == []
    else:
        assert asked == [best] and out["refined_score"] == out["scores"][best] and not out["refined"]


def test_consensus_in_many_chunks(ctx, monkeypatch):
    """candidate chunks of 7: the double-buffered hand-over, many chunks per level, the same consensus"""
    z, seqs, members = _load("syn8")
    monkeypatch.setenv("KA_ENS_CHUNK", "7")
    e = _ens(ctx, seqs, members)
    for m in (1, 3):
        assert [x.decode() for x in e.consensus(seqs, m)] == [str(x) for x in z["cons%d" % m]]
        assert e.stats()["chunks"] > 10
    e.close()


def _check_letter_case_and_gap_byte(ctx, seqs, members):
    """lower-case letters and '.' gaps are the same residues and gaps: equal scores, confidences and consensus columns"""
    other = [[r.lower().replace("-", ".") for r in m] for m in members]
    a, b = _ens(ctx, seqs, members), _ens(ctx, seqs, other)
    for rows, orows in zip(members, other):
        assert a.score(rows) == b.score(orows) == a.score(orows)
    ra, ca = a.confidence(members[0])
    rb, cb = b.confidence(other[0])
    assert np.array_equal(ra, rb) and np.array_equal(ca, cb)
    assert a.consensus(seqs, 2) == b.consensus(seqs, 2)
    a.close()
    b.close()


# alignment widths by seed: the last block of 64 columns partly filled (11, 12, 13) and full (14)
LIVE_WIDTH = {11: 100, 12: 77, 13: 125, 14: 128}


@pytest.mark.parametrize("seed,n,length,runs", [(11, 64, 80, 8), (12, 128, 60, 5), (13, 40, 100, 16), (14, 48, 101, 6)])
def test_stage_live_against_the_reference(ctx, seed, n, length, runs):
    import make_golden_ensemble as mg
    if not mg.available():
        pytest.skip("oracle/_ref not built")
    seqs, members = mg.synthetic(n, length, runs, seed, moves=10)
    assert len(members[0][0]) == LIVE_WIDTH[seed]
    _check_letter_case_and_gap_byte(ctx, seqs, members)
    mins = sorted({1, 2, ensemble_auto(runs), runs})
    want = mg.reference_stage(seqs, members, mins)
    _check_stage(ctx, want, seqs, members)


def test_bfs_queue_truncation_against_the_reference(ctx):
    """large enough that the reachability search's 4096-set queue fills: the replay stays the reference's"""
    import make_golden_ensemble as mg
    if not mg.available():
        pytest.skip("oracle/_ref not built")
    seqs, members = mg.synthetic(128, 300, 8, 21, moves=8)
    want = mg.reference_stage(seqs, members, [3])
    e = _ens(ctx, seqs, members)
    assert [x.decode() for x in e.consensus(seqs, 3)] == [str(x) for x in want["cons3"]]
    assert e.stats()["bfs_truncations"] > 0
    e.close()


@pytest.mark.parametrize("runs", [3, 8])
def test_end_to_end_against_kalign_ensemble(ctx, runs):
    """members from Context.run_encoded at the ensemble's parameters (gap penalties scaled per member, guide-tree noise
    from the reference's RNG), the refinement re-run from run_encoded(refine=2), then finish_ensemble: the rows and
    confidences of kalign_ensemble's tail on the same members, restated over the reference's POAR functions
    (make_golden_ensemble.reference_finish, which reproduces kalign_ensemble on the reference's own members: ens_real_*)"""
    import make_golden_ensemble as mg
    from kalign_amd import ensemble, synth
    from oracle import refdrv
    if not mg.available():
        pytest.skip("oracle/_ref not built")
    seqs = synth.dssim(64, 120, seed=5)
    seed = 42
    job = refdrv.RefJob(seqs, use_seq_weights=0.0)
    base = (job.gpo, job.gpe, job.tgpe)
    ranks = [int(r) for r in job.ranks]
    letters = [seqs[r] for r in ranks]
    n = len(seqs)

    def member(k, refine=0):
        (g, e, t), tseed, noise = mg.member_params(base, k, seed)
        scal = np.array([g, e, t, job.dist_scale, job.vsm_amax, 0.0], np.float32)
        dms = refdrv.noise_multipliers(tseed, noise, n * min(32, n)) if tseed and noise > 0 else None
        rows = ctx.run_encoded(job.tree_codes, job.codes, letters, job.subm, scal, dm_scale=dms, refine=refine)
        out = [None] * n
        for i, r in enumerate(ranks):
            out[r] = rows[i]
        return out
    members = [member(k) for k in range(runs)]
    refined = {}

    def rerun(k):
        if k not in refined:
            refined[k] = member(k, refine=2)
        return refined[k]
    got = ensemble.finish_ensemble(ctx, members, seqs, rerun_refined=rerun)
    job.close()
    rows, res, col, decision = mg.reference_finish(seqs, [[x.decode() for x in m] for m in members],
                                                   lambda k: [x.decode() for x in rerun(k)])
    assert got["use_consensus"] == (decision == "consensus") and got["refined"] == (decision == "refined")
    assert [x.decode() for x in got["rows"]] == rows
    assert np.array_equal(got["residue_confidence"], res) and np.array_equal(got["column_confidence"], col)


def ensemble_auto(runs):
    from kalign_amd import ensemble
    return ensemble.auto_min_support(runs)


def test_errors(ctx):
    from kalign_amd import KalignAmdError
    with pytest.raises(KalignAmdError, match="4096"):
        ctx.ensemble([10, 4097], 3)
    ctx.ensemble([10, 4096], 3).close()
    with pytest.raises(KalignAmdError, match="n_runs"):
        ctx.ensemble([10, 12], 33)
    with pytest.raises(KalignAmdError, match="n_runs"):
        ctx.ensemble([10, 12], 0)


def test_context_closed_first():
    """an Ensemble borrows its context's stream: closing the context closes the ensemble first"""
    import kalign_amd
    from kalign_amd import KalignAmdError
    c = kalign_amd.Context(0)
    e = c.ensemble([3, 2], 1)
    e.add_member(0, ["ACD", "A-C"])
    c.close()
    assert e.h is None
    e.close()
    with pytest.raises(KalignAmdError, match="closed"):
        c.ensemble([3, 2], 1)


def test_error_rows(ctx):
    from kalign_amd import KalignAmdError
    e = ctx.ensemble([3, 2], 2)
    e.add_member(0, ["ACD-", "A--C"])
    with pytest.raises(KalignAmdError, match="row 1 holds 3 letters"):
        e.add_member(1, ["ACD-", "A-YC"])
    with pytest.raises(KalignAmdError, match="not added"):
        e.score(["ACD-", "A--C"])
    e.add_member(1, ["AC-D", "-A-C"])
    # a width that does not fit the stride, through the C ABI
    rows = np.frombuffer(b"ACD-A--C", np.uint8)
    rc = ctx.L.ka_ens_add_member(e.h, 0, rows.ctypes.data_as(C.c_void_p), 4, 5)
    assert rc != 0 and b"stride" in ctx.L.ka_last_error()
    s, v = e.score(["ACD-", "A--C"])
    assert (s, v) == (0, 0.0)                 # one pair, (A, A) in column 0: member 0 only, support 1
    e.close()


def _numpy_sum(members, rows):
    """sum over the residue pairs of `rows` of (support - 1), support = members with the two residues in one column"""
    n = len(rows)

    def cols(r):
        a = np.frombuffer(r.encode() if isinstance(r, str) else r, np.uint8)
        return np.flatnonzero(((a | 32) >= ord("a")) & ((a | 32) <= ord("z")))
    mcol = [[cols(r) for r in m] for m in members]          # [k][s] -> column of each residue
    x = np.array([np.frombuffer(r.encode() if isinstance(r, str) else r, np.uint8) for r in rows])
    isres = ((x | 32) >= ord("a")) & ((x | 32) <= ord("z"))
    resx = np.where(isres, np.cumsum(isres, axis=1) - 1, -1)
    total = 0
    for i in range(n):
        for j in range(i + 1, n):
            both = (resx[i] >= 0) & (resx[j] >= 0)
            ri, rj = resx[i][both], resx[j][both]
            sup = np.zeros(len(ri), np.int64)
            for m in mcol:
                sup += m[i][ri] == m[j][rj]
            total += int((sup - 1).sum())
    return total


def test_property_2048x300x8(ctx):
    """the workload's size on the device only: the consensus is an alignment of the inputs, confidences in [0, 1], and
    S(member 0) on a 64-sequence subsample equals a numpy recount"""
    import make_golden_ensemble as mg
    seqs, members = mg.synthetic(2048, 300, 8, 7, moves=8)
    e = _ens(ctx, seqs, members)
    rows = e.consensus(seqs, 3)
    assert len({len(r) for r in rows}) == 1
    for s, r in zip(seqs, rows):
        assert bytes(b for b in r if b != ord("-")).decode() == s
    res, col = e.confidence(rows)
    assert res.min() >= 0.0 and res.max() <= 1.0 and col.min() >= 0.0 and col.max() <= 1.0
    st = e.stats()
    assert st["level_candidates"] and st["chunks"] >= 1
    e.close()
    pick = np.random.default_rng(3).choice(2048, 64, replace=False)
    sub = [[m[i] for i in pick] for m in members]
    e = _ens(ctx, [seqs[i] for i in pick], sub)
    assert e.score(sub[0])[0] == _numpy_sum(sub, sub[0])
    e.close()
