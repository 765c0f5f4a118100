"""GPU: the ensemble consensus stage for a batch of families in one pass (ka_ens_fam, Context.family_ensemble,
ensemble.finish_ensembles) -- against the reference's stored results (tests/golden/ens_*.npz), against the one-family
Ensemble with == at the edges of the launch geometry, with candidate chunks of whole families, with launch and
synchronisation counts that do not grow with the batch, and live against oracle/_ref where it is built."""
import glob
import os
import sys

import numpy as np
import pytest

from util import GOLDEN

pytestmark = pytest.mark.gpu

CASES = sorted(os.path.basename(f)[4:-4] for f in glob.glob(os.path.join(GOLDEN, "ens_*.npz")))
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


def _batch(ctx, fams):
    """fams: [(seqs, members)] with one number of members -> a FamilyEnsemble with every member added"""
    runs = len(fams[0][1])
    e = ctx.family_ensemble([[len(s) for s in seqs] for seqs, _ in fams], runs)
    for k in range(runs):
        e.add_member(k, [m[k] for _, m in fams])
    return e


def _alone(ctx, seqs, members, min_support, chosen=None):
    """the one-family Ensemble on one family: member scores, consensus rows, their score, confidences of `chosen` (member 0)"""
    e = ctx.ensemble([len(s) for s in seqs], len(members))
    for k, rows in enumerate(members):
        e.add_member(k, rows)
    out = dict(scores=[e.score(rows) for rows in members], cons=e.consensus(seqs, min_support))
    out["cons_score"] = e.score(out["cons"])
    out["conf"] = e.confidence(members[0] if chosen is None else chosen)
    out["cons_conf"] = e.confidence(out["cons"])
    e.close()
    return out


def _check_equal(ctx, fams, min_support, n_threads=4):
    """every value of the batch == the one-family handle's: sums, scores, rows, confidences"""
    runs = len(fams[0][1])
    ms = [min_support] * len(fams) if isinstance(min_support, int) else list(min_support)
    e = _batch(ctx, fams)
    sums, scores = e.score_members()
    cons = e.consensus([s for s, _ in fams], ms, n_threads)
    csum, cscore = e.score(cons)
    conf0 = e.confidence([m[0] for _, m in fams])
    cconf = e.confidence(cons)
    st = e.stats()
    e.close()
    for f, (seqs, members) in enumerate(fams):
        w = _alone(ctx, seqs, members, ms[f])
        assert [(int(sums[k, f]), float(scores[k, f])) for k in range(runs)] == w["scores"], f
        assert cons[f] == w["cons"], f
        assert (int(csum[f]), float(cscore[f])) == w["cons_score"], f
        for got, want in ((conf0[f], w["conf"]), (cconf[f], w["cons_conf"])):
            assert got[0].shape == want[0].shape and got[0].tobytes() == want[0].tobytes(), f
            assert got[1].tobytes() == want[1].tobytes(), f
    return st


# ---- the reference's stored results ------------------------------------------------------------------------------------------

def _by_runs():
    groups = {}
    for name in CASES:
        groups.setdefault(int(np.load(os.path.join(GOLDEN, "ens_%s.npz" % name))["members"].shape[0]), []).append(name)
    return groups


@pytest.mark.parametrize("runs", sorted(_by_runs()))
def test_stage_against_golden(ctx, runs):
    """the cases of one member count as one batch, each family against its stored values (test_gpu_ensemble_stage._check_stage's
    tolerances: scores rel=1e-9 -- the reference adds in double --, everything else ==)"""
    names = _by_runs()[runs]
    loaded = [_load(n) for n in names]
    fams = [(seqs, members) for _, seqs, members in loaded]
    e = _batch(ctx, fams)
    scores = e.score_members()[1]
    conf0 = e.confidence([m[0] for _, m in fams])
    for f, (z, _, _) in enumerate(loaded):
        for k in range(runs):
            assert float(scores[k, f]) == pytest.approx(float(z["scores"][k]), rel=1e-9, abs=1e-9), (names[f], k)
        assert np.array_equal(conf0[f][0], z["m0_res_conf"]) and np.array_equal(conf0[f][1], z["m0_col_conf"]), names[f]
    # the stored thresholds: position p of every family's list in one consensus call (a family with fewer repeats its last)
    mins = [[int(m) for m in z["min_supports"]] for z, _, _ in loaded]
    for p in range(max(len(m) for m in mins)):
        ms = [m[min(p, len(m) - 1)] for m in mins]
        cons = e.consensus([s for s, _ in fams], ms)
        cscore = e.score(cons)[1]
        cconf = e.confidence(cons)
        for f, (z, _, _) in enumerate(loaded):
            m = ms[f]
            assert [x.decode() for x in cons[f]] == [str(x) for x in z["cons%d" % m]], (names[f], m)
            assert float(cscore[f]) == pytest.approx(float(z["cons%d_score" % m]), rel=1e-9, abs=1e-9), (names[f], m)
            assert np.array_equal(cconf[f][0], z["cons%d_res_conf" % m]), (names[f], m)
            assert np.array_equal(cconf[f][1], z["cons%d_col_conf" % m]), (names[f], m)
    e.close()


def test_finish_ensembles_equals_kalign_ensemble(ctx):
    """the ens_real_* cases of one member count through finish_ensembles, with their stored refined re-runs: the rows and
    confidences kalign_ensemble gave for each"""
    from kalign_amd import ensemble
    real = [n for n in CASES if n.startswith("real_")]
    runs = max(_by_runs(), key=lambda r: sum(n in real for n in _by_runs()[r]))
    names = [n for n in _by_runs()[runs] if n in real]
    assert len(names) >= 2, names
    loaded = [_load(n) for n in names]
    refined = [[[str(r) for r in m] for m in z["refined"]] for z, _, _ in loaded]
    member_rows = [[members[k] for _, _, members in loaded] for k in range(runs)]
    asked = []

    def rerun(pairs):
        asked.extend(pairs)
        return [refined[f][k] for f, k in pairs]
    outs = ensemble.finish_ensembles(ctx, member_rows, [seqs for _, seqs, _ in loaded], rerun_refined=rerun)
    for f, (z, seqs, members) in enumerate(loaded):
        assert [x.decode() for x in outs[f]["rows"]] == [str(x) for x in z["ens_rows"]], names[f]
        assert np.array_equal(outs[f]["residue_confidence"], z["ens_res_conf"]), names[f]
        assert np.array_equal(outs[f]["column_confidence"], z["ens_col_conf"]), names[f]
        one = ensemble.finish_ensemble(ctx, members, seqs, rerun_refined=lambda k, f=f: refined[f][k])
        for key in ("scores", "best_k", "use_consensus", "consensus_score", "refined_score", "refined", "rows"):
            assert outs[f][key] == one[key], (names[f], key)
    assert asked == [(f, o["best_k"]) for f, o in enumerate(outs) if not o["use_consensus"]]
    # an explicit threshold: the consensus, no selection
    m = int(loaded[0][0]["min_supports"][0])
    outs = ensemble.finish_ensembles(ctx, member_rows, [seqs for _, seqs, _ in loaded], min_support=m)
    for f, (z, seqs, members) in enumerate(loaded):
        one = ensemble.finish_ensemble(ctx, members, seqs, min_support=m)
        assert outs[f]["use_consensus"] and outs[f]["rows"] == one["rows"]
        assert outs[f]["residue_confidence"].tobytes() == one["residue_confidence"].tobytes()


# ---- equality with the one-family Ensemble at the edges of the geometry ------------------------------------------------------

ALPHABET = list("ACDEFGHIKLMNPQRSTVWY")


def _family(rng, lens, runs, widths, style=0):
    """sequences of these lengths and `runs` members of them: member k is `widths[k % len(widths)]` columns wide (at least the
    longest sequence); every row keeps a base placement of its residues or draws a new one, so support levels from 1 to runs
    occur.  style 1: lower-case letters and '.' gaps in the odd members."""
    seqs = ["".join(rng.choice(ALPHABET, n)) for n in lens]
    members = []
    base = {}
    for k in range(runs):
        W = max(widths[k % len(widths)], max(lens))
        rows = []
        for s, q in enumerate(seqs):
            if (W, s) not in base:
                base[(W, s)] = np.sort(rng.choice(W, len(q), replace=False))
            cols = base[(W, s)] if rng.random() < 0.6 else np.sort(rng.choice(W, len(q), replace=False))
            row = np.full(W, ord("-"), np.uint8)
            row[cols] = np.frombuffer(q.encode(), np.uint8)
            r = row.tobytes().decode()
            rows.append(r.lower().replace("-", ".") if style and k % 2 else r)
        members.append(rows)
    return seqs, members


def _edge_batch(runs):
    rng = np.random.default_rng(1000 + runs)
    fams = []
    for n in (2, 3, 15, 16, 17, 33):                              # both sides of KA_ENS_JCHUNK = 16, and three j chunks
        lens = [int(x) for x in rng.integers(20, 50, n)]
        lens[0] = 3                                               # much shorter than its family
        fams.append(_family(rng, lens, runs, [64, 70], style=n % 2))
    fams.append(_family(rng, [1, 63, 64, 65], runs, [128, 129, 65], style=1))      # last block of 64 columns full and partly filled
    fams.append(_family(rng, [1], runs, [1]))                                     # a family of one sequence: no pair at all
    return fams


@pytest.mark.parametrize("runs", [1, 2, 8, 9, 32])
def test_equal_to_the_one_family_handle_at_the_edges(ctx, runs):
    """n_runs on both sides of the RM = 8 / 32 split; at 32 members one family reads the member columns where they lie
    ((3 + 32) * 471 * 4 > 64 KiB) next to families that stage them in LDS"""
    fams = _edge_batch(runs)
    if runs == 32:
        rng = np.random.default_rng(7)
        fams.insert(3, _family(rng, [471, 200, 330, 8], runs, [500, 512], style=1))
        assert (3 + runs) * 471 * 4 > 65536
    ms = [1 + f % max(1, runs) for f in range(len(fams))]
    _check_equal(ctx, fams, ms)


def test_score_members_equals_score_and_none_skips(ctx):
    fams = _edge_batch(3)
    e = _batch(ctx, fams)
    sums, scores = e.score_members()
    for k in range(3):
        s, v = e.score([m[k] for _, m in fams])
        assert s.tolist() == sums[k].tolist() and v.tolist() == scores[k].tolist()
    rows = [m[1] for _, m in fams]
    for skipped in ([0], [2, 5], list(range(1, len(fams)))):
        s, v = e.score([None if f in skipped else r for f, r in enumerate(rows)])
        for f in range(len(fams)):
            assert (s[f], v[f]) == ((0, 0.0) if f in skipped else (sums[1, f], scores[1, f])), (skipped, f)
    e.close()


def test_min_support_per_family(ctx):
    """thresholds that differ inside one batch: 1, 2, the automatic one, n_runs, and one above n_runs (no candidates)"""
    from kalign_amd import ensemble
    fams = _edge_batch(8)
    choice = [1, 2, ensemble.auto_min_support(8), 8, 9]
    _check_equal(ctx, fams, [choice[f % len(choice)] for f in range(len(fams))], n_threads=16)


# ---- chunks, launches -------------------------------------------------------------------------------------------------------

def test_consensus_in_many_chunks(ctx, monkeypatch):
    """KA_ENS_CHUNK=7 as test_gpu_ensemble_stage.test_consensus_in_many_chunks sets it: chunks of whole families, level by
    level -- the same rows from more chunks than there are families"""
    import make_golden_ensemble as mg
    z, seqs8, members8 = _load("syn8")
    fams = [(seqs8, members8)] + [mg.synthetic(3 + f, 10 + 3 * f, 8, 50 + f, moves=3) for f in range(6)]
    seqs = [s for s, _ in fams]
    e = _batch(ctx, fams)
    e.score_members()                                            # (the members' maps: not the consensus' launches)
    want = e.consensus(seqs, 1)
    whole = e.stats()
    assert 1 <= whole["chunks"] <= 8                             # (one per support level that holds a candidate)
    e.close()
    assert [x.decode() for x in want[0]] == [str(x) for x in z["cons1"]]
    monkeypatch.setenv("KA_ENS_CHUNK", "7")
    e = _batch(ctx, fams)
    e.score_members()
    assert e.consensus(seqs, 1) == want
    st = e.stats()
    assert st["chunks"] > len(fams) and st["candidates"] == whole["candidates"]
    assert st["consensus_launches"] == 2 + st["chunks"] and st["consensus_syncs"] == whole["consensus_syncs"] - whole["chunks"] + st["chunks"]
    e.close()


def test_small_families_share_a_chunk(ctx, monkeypatch):
    """one member, so one support level: twelve small families under a cap of three average families"""
    import make_golden_ensemble as mg
    small = [mg.synthetic(2, 6, 1, 70 + f, moves=2) for f in range(12)]
    seqs = [s for s, _ in small]
    e = _batch(ctx, small)
    want = e.consensus(seqs, 1)
    st = e.stats()
    assert st["chunks"] == 1
    e.close()
    monkeypatch.setenv("KA_ENS_CHUNK", str(int(3 * st["candidates"] / len(small))))
    e = _batch(ctx, small)
    assert e.consensus(seqs, 1) == want
    assert 1 < e.stats()["chunks"] < len(small)
    e.close()


def test_a_family_above_the_cap_is_a_chunk_of_its_own(ctx, monkeypatch):
    """one member, so one support level; a cap between the smallest and the largest family's candidate count"""
    import make_golden_ensemble as mg
    fams = [mg.synthetic(3, 8, 1, 90, moves=2), mg.synthetic(12, 40, 1, 91, moves=4), mg.synthetic(3, 8, 1, 92, moves=2),
            mg.synthetic(3, 8, 1, 93, moves=2)]
    seqs = [s for s, _ in fams]
    counts = []
    for fam in fams:
        e = _batch(ctx, [fam])
        e.consensus([fam[0]], 1)
        counts.append(e.stats()["candidates"])
        e.close()
    assert counts[1] > 2 * (counts[0] + counts[2] + counts[3]) and min(counts) > 0
    want = [_alone(ctx, s, m, 1)["cons"] for s, m in fams]
    monkeypatch.setenv("KA_ENS_CHUNK", str(max(counts[0], counts[2] + counts[3])))
    e = _batch(ctx, fams)
    assert e.consensus(seqs, 1) == want
    assert e.stats()["chunks"] == 3                               # {0}, {1} alone, {2, 3}
    e.close()


def test_launches_do_not_grow_with_the_batch(ctx):
    """the same four families once and sixteen times over: the same support levels hold candidates, so the same chunks"""
    import make_golden_ensemble as mg
    from kalign_amd import api
    keys = [k for k in api.ENS_FAM_STATS if k.endswith("_launches") or k.endswith("_syncs")] + ["chunks"]
    four = [mg.synthetic(5, 20, 8, 200 + f, moves=3) for f in range(4)]
    seen = []
    for times in (1, 16):
        fams = four * times
        e = _batch(ctx, fams)
        e.score_members()
        cons = e.consensus([s for s, _ in fams], 3)
        e.score(cons)
        e.confidence(cons)
        st = e.stats()
        e.close()
        assert st["candidates"] > 0
        seen.append({k: st[k] for k in keys})
    assert seen[0] == seen[1], seen
    assert seen[0]["consensus_launches"] == 2 + seen[0]["chunks"] and seen[0]["score_members_launches"] == 8 + 8
    assert seen[0]["score_launches"] == 2 and seen[0]["confidence_launches"] == 4


# ---- property, errors, live reference --------------------------------------------------------------------------------------

def test_property_64_families(ctx):
    """64 families x 32 x ~100 residues x 8 members: every family's scores, consensus and confidences equal a loop of
    one-family handles"""
    import make_golden_ensemble as mg
    fams = [mg.synthetic(32, 100, 8, 300 + f, moves=8) for f in range(64)]
    st = _check_equal(ctx, fams, 3, n_threads=16)
    assert st["candidates"] > 64 * 32 * 31 // 2 and 1 <= st["chunks"] <= 6


def test_errors_leave_the_handle_usable(ctx):
    from kalign_amd import KalignAmdError
    fams = _edge_batch(2)
    e = ctx.family_ensemble([[len(s) for s in seqs] for seqs, _ in fams], 2)
    e.add_member(0, [m[0] for _, m in fams])
    for call in (e.score_members, lambda: e.score([m[0] for _, m in fams]), lambda: e.consensus([s for s, _ in fams], 1),
                 lambda: e.confidence([m[0] for _, m in fams])):
        with pytest.raises(KalignAmdError, match="member 1 not added"):
            call()
    bad = [list(m[1]) for _, m in fams]
    bad[3][1] = bad[3][1][:-1] + ("A" if bad[3][1][-1] in "-." else "-")
    with pytest.raises(KalignAmdError, match=r"ka_ens_fam_add_member: family 3: row 1 holds \d+ letters, its sequence \d+ \(every alignment"):
        e.add_member(1, bad)
    e.add_member(1, [m[1] for _, m in fams])
    good = e.score([m[0] for _, m in fams])
    with pytest.raises(KalignAmdError, match=r"ka_ens_fam_score: family 3: row 1 holds"):
        e.score(bad)
    with pytest.raises(KalignAmdError, match=r"ka_ens_fam_confidence: family 3: row 1 holds"):
        e.confidence(bad)
    with pytest.raises(KalignAmdError, match="min_support 0"):
        e.consensus([s for s, _ in fams], 0)
    with pytest.raises(KalignAmdError, match="n_threads 17"):
        e.consensus([s for s, _ in fams], 1, n_threads=17)
    again = e.score([m[0] for _, m in fams])
    assert good[0].tolist() == again[0].tolist() and good[1].tolist() == again[1].tolist()
    seqs, members = fams[3]
    assert e.consensus([s for s, _ in fams], 1)[3] == _alone(ctx, seqs, members, 1)["cons"]
    e.close()
    with pytest.raises(KalignAmdError, match="closed"):
        e.score([m[0] for _, m in fams])


def test_context_closed_first():
    """a FamilyEnsemble borrows its context's stream: closing the context closes it first"""
    import kalign_amd
    from kalign_amd import KalignAmdError
    c = kalign_amd.Context(0)
    e = c.family_ensemble([[3, 2], [1]], 1)
    e.add_member(0, [["ACD", "A-C"], ["W"]])
    c.close()
    assert e.h is None
    e.close()
    with pytest.raises(KalignAmdError, match="closed"):
        c.family_ensemble([[3, 2]], 1)


def test_live_against_the_reference(ctx):
    import make_golden_ensemble as mg
    from kalign_amd import ensemble
    if not mg.available():
        pytest.skip("oracle/_ref not built")
    runs = 5
    fams = [mg.synthetic(n, length, runs, seed, moves=6) for n, length, seed in ((9, 30, 31), (17, 45, 32), (4, 64, 33))]
    mins = sorted({1, ensemble.auto_min_support(runs), runs})
    want = [mg.reference_stage(seqs, members, mins) for seqs, members in fams]
    e = _batch(ctx, fams)
    scores = e.score_members()[1]
    conf0 = e.confidence([m[0] for _, m in fams])
    for f, w in enumerate(want):
        for k in range(runs):
            assert float(scores[k, f]) == pytest.approx(float(w["scores"][k]), rel=1e-9, abs=1e-9)
        assert np.array_equal(conf0[f][0], w["m0_res_conf"]) and np.array_equal(conf0[f][1], w["m0_col_conf"])
    for m in mins:
        cons = e.consensus([s for s, _ in fams], m)
        cscore = e.score(cons)[1]
        cconf = e.confidence(cons)
        for f, w in enumerate(want):
            assert [x.decode() for x in cons[f]] == [str(x) for x in w["cons%d" % m]], (f, m)
            assert float(cscore[f]) == pytest.approx(float(w["cons%d_score" % m]), rel=1e-9, abs=1e-9)
            assert np.array_equal(cconf[f][0], w["cons%d_res_conf" % m]) and np.array_equal(cconf[f][1], w["cons%d_col_conf" % m])
    e.close()
