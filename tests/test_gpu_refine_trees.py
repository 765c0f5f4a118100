"""GPU: KALIGN_REFINE_CONFIDENT with a median per tree of a forest job (ka_tree_refine_trees, Context.tree_refine_trees) against
the real reference's refine_alignment goldens (tests/golden/refine_*_conf*.npz, made from the reference itself): several of them
as ONE forest job, every tree refined by the median of its own edges.  ka_tree_refine pools the median over the job; the forest
below is one where that marks another edge, so a pooled rule cannot pass."""
import numpy as np
import pytest

from util import Golden, refine_cases

pytestmark = pytest.mark.gpu

CONF = [n for n in refine_cases() if "_conf" in n]
REC_FIELDS = ("a", "b", "c", "len_a", "len_b", "nsip_a", "nsip_b", "plen", "kind", "swapped", "meet", "transition",
              "gap_scale", "subm_off", "score", "confidence", "prof_hash", "fhash", "bhash")


@pytest.fixture(scope="module")
def ctx():
    import kalign_amd
    c = kalign_amd.Context(0)
    yield c
    c.close()


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def upload_forest(ctx, gs):
    from kalign_amd import guide
    for g in gs[1:]:
        assert np.array_equal(g.subm, gs[0].subm) and np.array_equal(g.scal, gs[0].scal) and int(g.n_anchors) == int(gs[0].n_anchors)
    codes, tasks, dist, spans = guide.forest([(g.codes, g.tasks, g.seq_distances) for g in gs])
    ctx.tree_upload(codes, tasks, gs[0].subm, gs[0].scal, dist)
    if int(gs[0].n_anchors) > 0:
        ctx.tree_build_consistency(int(gs[0].n_anchors), float(gs[0].weight))
    return spans


def check_trees(gs, spans, recs, gaps):
    """every tree of the forest against its own golden: gap arrays, profile lengths, the kept trials' confidences as bits"""
    for g, (s0, t0, ns, nt) in zip(gs, spans):
        for got, want in zip(gaps[s0:s0 + ns], g.gaps_list()):
            assert np.array_equal(got, want)
        for t in range(nt):
            assert recs[t0 + t].plen == g.plen_after[g.tasks[t][2]], t
        assert np.array_equal(bits([r.confidence for r in recs[t0:t0 + nt]]), bits(g.conf_after))
        assert int(g.n_differ) > 0


def snapshot(ctx):
    """what a download holds: every field of every record but where its path lies (the path arena is handed out in the order
    tasks finish), every task's coded path, every sequence's gaps"""
    recs, paths, gaps = ctx.tree_download()
    return ([tuple(getattr(r, f) for f in REC_FIELDS) for r in recs],
            [paths[r.path_off:r.path_off + r.plen + 2].copy() for r in recs], [g.copy() for g in gaps])


def same(a, b):
    return a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1], b[1])) and all(np.array_equal(x, y) for x, y in zip(a[2], b[2]))


@pytest.fixture(scope="module")
def two():
    return [Golden("refine_BB30014_conf"), Golden("refine_prot32x200_conf")]


def test_forest_of_two_goldens(ctx, two):
    ga, gb = two
    assert len(ga.tasks) == 43 and len(gb.tasks) == 31 and int(ga.n_anchors) == 0 and int(ga.mode) == 2 and int(gb.mode) == 2
    conf = np.concatenate([ga.conf_before, gb.conf_before]).astype(np.float32)
    med = [np.median(ga.conf_before), np.median(gb.conf_before)]
    assert all(m.dtype == np.float32 for m in med)
    # the case discriminates, by the goldens alone: the pooled median marks another set of edges than the trees' own medians,
    # and refining changes the confidence of every edge the two rules disagree on
    per_tree = np.concatenate([ga.conf_before <= med[0], gb.conf_before <= med[1]])
    pooled = conf <= np.median(conf)
    differ = np.nonzero(per_tree != pooled)[0]
    assert len(differ) >= 1
    after = np.concatenate([ga.conf_after, gb.conf_after])
    assert all(bits(after[t]) != bits(conf[t]) for t in differ)
    for conf_in in (conf, None):                                  # None: the device's own mode-4 pass supplies the confidences
        spans = upload_forest(ctx, two)
        tree_of, thr = ctx.tree_refine_trees(2, conf_in)
        recs, _, gaps = ctx.tree_download()
        assert list(tree_of) == [0] * 43 + [1] * 31
        assert np.array_equal(bits(thr), bits(med))
        check_trees(two, spans, recs, gaps)


def test_adaptive_budget_and_consistency(ctx):
    """the adaptive golden twice as one forest (K = 3 for both): adaptive trial counts and the consistency bonus under the new entry"""
    g = Golden("refine_cons_prot24_conf_adaptive")
    assert int(g.mode) == (2 | 256) and int(g.n_anchors) == 3 and float(g.weight) == 2.0
    spans = upload_forest(ctx, [g, g])
    tree_of, thr = ctx.tree_refine_trees(2 | 256, np.concatenate([g.conf_before, g.conf_before]))
    recs, _, gaps = ctx.tree_download()
    nt = len(g.tasks)
    assert list(tree_of) == [0] * nt + [1] * nt
    assert np.array_equal(bits(thr), bits([np.median(g.conf_before)] * 2))
    check_trees([g, g], spans, recs, gaps)


@pytest.mark.parametrize("name", CONF)
def test_single_tree_is_the_same_call(ctx, name):
    """on a job of one tree ka_tree_refine_trees and ka_tree_refine download identical records, paths and gaps -- and the golden's"""
    g = Golden(name)
    got = []
    for entry in (ctx.tree_refine_trees, ctx.tree_refine):
        upload_forest(ctx, [g])
        out = entry(int(g.mode), g.conf_before)
        got.append(snapshot(ctx))
        if entry == ctx.tree_refine_trees:
            assert not out[0].any() and np.array_equal(bits(out[1]), bits([np.median(g.conf_before)]))
    assert same(got[0], got[1])
    for a, want in zip(got[0][2], g.gaps_list()):
        assert np.array_equal(a, want)
    # ... and with the device's own confidences
    upload_forest(ctx, [g])
    ctx.tree_refine_trees(int(g.mode))
    assert same(snapshot(ctx), got[0])


@pytest.mark.parametrize("mode", [1, 3, 4])
def test_other_modes_equal_tree_refine(ctx, two, mode):
    got = []
    for entry in (ctx.tree_refine_trees, ctx.tree_refine):
        upload_forest(ctx, two)
        out = entry(mode)
        got.append(snapshot(ctx))
        if entry == ctx.tree_refine_trees:
            assert list(out[0]) == [0] * 43 + [1] * 31 and list(out[1]) == [0.0, 0.0]
    assert same(got[0], got[1])


def test_argument_errors(ctx, two):
    from kalign_amd.api import KalignAmdError
    upload_forest(ctx, two)
    for bad in (5, 0, 4 | 256, 3 | 256, 2 | (3 << 16), 2 | 512):
        for entry in (ctx.tree_refine_trees, ctx.tree_refine):
            with pytest.raises(KalignAmdError, match="mode must be|goes with"):
                entry(bad)
    with pytest.raises(KalignAmdError, match="one confidence per task"):
        ctx.tree_refine_trees(2, two[0].conf_before)
    import kalign_amd
    c = kalign_amd.Context(0)
    try:
        with pytest.raises(KalignAmdError, match="no uploaded job"):
            c._job = dict(ntasks=1)
            c.tree_refine_trees(2)
    finally:
        c.close()
    assert kalign_amd.load_library().ka_abi_version() >= 22
