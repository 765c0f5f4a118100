"""GPU: both ensemble handles (ka_ens_fam as a batch, ka_ens on each family alone) against the numpy restatement of the stage
(tests/ens_restate.py, itself held to the reference by tests/test_ens_restate.py) with == at the edges of the launch
geometry, and the one-family handle's count blocks (KA_ENS_COUNT_ROWS) against the reference's stored rows."""
import os

import numpy as np
import pytest

import ens_restate as er
from test_gpu_ensemble_families import _batch, _edge_batch, _family
from util import GOLDEN

pytestmark = pytest.mark.gpu


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


def _restated(seqs, members, min_support):
    """what both handles must give for one family: member sums, consensus rows, their sum, confidences of member 0 and of the rows"""
    t = er.Table.of_members(members, [len(s) for s in seqs])
    cons = t.consensus(seqs, min_support)
    return dict(sums=[t.score(rows) for rows in members], cons=cons, cons_sum=t.score(cons),
                conf=t.confidence(members[0]), cons_conf=t.confidence(cons))


def _same_conf(got, want):
    return got[0].shape == want[0].shape and got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


def _check_alone(ctx, seqs, members, min_support, want):
    e = ctx.ensemble([len(s) for s in seqs], len(members))
    for k, rows in enumerate(members):
        e.add_member(k, rows)
    assert [e.score(rows) for rows in members] == want["sums"]
    cons = e.consensus(seqs, min_support)
    assert cons == want["cons"]
    assert e.score(cons) == want["cons_sum"]
    assert _same_conf(e.confidence(members[0]), want["conf"]) and _same_conf(e.confidence(cons), want["cons_conf"])
    e.close()


@pytest.mark.parametrize("runs", [1, 2, 8, 9, 32])
def test_both_handles_equal_the_restatement_at_the_edges(ctx, runs):
    """test_equal_to_the_one_family_handle_at_the_edges' families (N on both sides of KA_ENS_JCHUNK, n_runs on both sides of the
    RM = 8 / 32 split, at 32 members a family whose member columns are not staged in LDS): each once in the batch, once alone"""
    fams = _edge_batch(runs)
    if runs == 32:
        fams.insert(3, _family(np.random.default_rng(7), [471, 200, 330, 8], runs, [500, 512], style=1))
        assert (3 + runs) * 471 * 4 > 65536
    ms = [1 + f % max(1, runs) for f in range(len(fams))]
    want = [_restated(seqs, members, ms[f]) for f, (seqs, members) in enumerate(fams)]
    e = _batch(ctx, fams)
    sums, scores = e.score_members()
    cons = e.consensus([s for s, _ in fams], ms, 4)
    csum, cscore = e.score(cons)
    conf0 = e.confidence([m[0] for _, m in fams])
    cconf = e.confidence(cons)
    e.close()
    for f, (seqs, members) in enumerate(fams):
        w = want[f]
        assert [(int(sums[k, f]), float(scores[k, f])) for k in range(runs)] == w["sums"], f
        assert cons[f] == w["cons"], f
        assert (int(csum[f]), float(cscore[f])) == w["cons_sum"], f
        assert _same_conf(conf0[f], w["conf"]) and _same_conf(cconf[f], w["cons_conf"]), f
        _check_alone(ctx, seqs, members, ms[f], w)


# ---- the one-family handle's count blocks -------------------------------------------------------------------------------------

def _blocks_ran(ctx, monkeypatch, make, seqs, rows):
    """KA_ENS_COUNT_ROWS is not ignored: under the default chunk cap a level leaves the device as one chunk per count block that
    holds a candidate, so more blocks give more chunks (and the same rows)"""
    monkeypatch.delenv("KA_ENS_COUNT_ROWS", raising=False)
    monkeypatch.delenv("KA_ENS_CHUNK", raising=False)
    e = make()
    want = e.consensus(seqs, 1)
    one = e.stats()
    e.close()
    assert 1 <= one["chunks"] <= len(one["level_candidates"])
    monkeypatch.setenv("KA_ENS_COUNT_ROWS", str(rows))
    e = make()
    assert e.consensus(seqs, 1) == want
    st = e.stats()
    e.close()
    assert st["level_candidates"] == one["level_candidates"]
    blocks = -(-len(seqs) // rows)
    assert one["chunks"] < st["chunks"] <= blocks * len(one["level_candidates"])


@pytest.mark.parametrize("name,rows", [("syn8", 5), ("syn8", 1), ("syn32", 3)])
def test_count_blocks_give_the_stored_rows(ctx, monkeypatch, name, rows):
    """syn8 has 24 sequences: blocks of 5, 5, 5, 5, 4 rows end inside a j chunk of 16; syn32 is the RM = 32 form.  The levels
    still go highest first over all rows: the stored consensus, from many chunks"""
    z, seqs, members = _load(name)

    def make():
        e = ctx.ensemble([len(s) for s in seqs], len(members))
        for k, r in enumerate(members):
            e.add_member(k, r)
        return e
    _blocks_ran(ctx, monkeypatch, make, seqs, rows)
    monkeypatch.setenv("KA_ENS_COUNT_ROWS", str(rows))
    monkeypatch.setenv("KA_ENS_CHUNK", "7")
    e = make()
    for m in (1, 3):
        assert [x.decode() for x in e.consensus(seqs, m)] == [str(x) for x in z["cons%d" % m]], m
        assert e.stats()["chunks"] > 10
    e.close()


@pytest.mark.parametrize("runs", [8, 9])
def test_a_last_block_of_one_row_without_pairs(ctx, monkeypatch, runs):
    """N = 17 in blocks of 16: the second block is row 16 alone, which has no pair j > i"""
    seqs, members = _edge_batch(runs)[4]
    assert len(seqs) == 17
    monkeypatch.setenv("KA_ENS_COUNT_ROWS", "16")
    for m in (1, runs):
        _check_alone(ctx, seqs, members, m, _restated(seqs, members, m))


@pytest.mark.parametrize("rows", [5, 1])
def test_count_blocks_of_a_table_backed_handle(ctx, monkeypatch, rows):
    """a handle opened from syn8's table counts its levels through the same block function"""
    from poar_restate import poar_image
    z, seqs, members = _load("syn8")
    image = poar_image(members)

    def make():
        return ctx.ensemble_from_table([len(s) for s in seqs], image=image)
    _blocks_ran(ctx, monkeypatch, make, seqs, rows)
    monkeypatch.setenv("KA_ENS_COUNT_ROWS", str(rows))
    monkeypatch.setenv("KA_ENS_CHUNK", "7")
    e = make()
    for m in (1, 3):
        assert [x.decode() for x in e.consensus(seqs, m)] == [str(x) for x in z["cons%d" % m]], m
        assert e.stats()["chunks"] > 10
    e.close()
