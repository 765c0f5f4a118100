"""The profile merge (ka_update_profile) and the leaf records (ka_make_leaf_profile, ka_leaf_rec4), record by record: every
non-root node's (plen + 2) x 64 floats against the oracle's update_n along the same coded path, as uint32 -- a difference names
the job, the mode, the node, the first differing column and field and that column's op code.

The jobs are tests/merge_jobs.py's: tiny trees whose paths are planned (terminal gap runs at both ends, gap runs of 1, 2 and 5 or
more columns inside either operand, profile operands that arrive with gap columns) and whose lengths put the merge's item walk
either side of a stride and of a batched trip; tests/test_merge_inputs.py proves on the host that they are, and that the recipe
is the oracle's and the real reference's profile.  Every form of the merge runs: the batched loop in its four instances (which
operand is a sequence made from its residue) and the one-item loop it replaced (KA_MERGE = 0 / 1 / 3 / 7), on a cluster and on
one workgroup, elem() under sequence weights, the two-step adjustment of refined paths, and -- as forests -- the 4-wave kernel
and the 128-register units' lean build."""
import numpy as np
import pytest

import merge_jobs as mj
from test_gpu_parity import EXACT
from test_gpu_strip_edges import FOREST, _same

pytestmark = pytest.mark.gpu

JOBS = mj.jobs()
PROFILE_JOBS = [j for j in JOBS if j[0] != "ss"]
# A refined edge's record: EXACT -- the top-level meetup (meet, transition, score) is the baseline trial's, in the oracle and on
# the device -- without fhash / bhash, the hashes of the debug rows, which only a first pass records (a refinement pass leaves
# them 0), and with the kept trial's confidence, which a refinement pass adds up in the reference's order: the same float
REFINED = [f for f in EXACT if f not in ("fhash", "bhash")] + ["confidence"]


@pytest.fixture(scope="module")
def ctx():
    import kalign_amd
    c = kalign_amd.Context(0)
    yield c
    c.close()


def _set(monkeypatch, mode):
    for k in mj.MODE_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in mode.items():
        monkeypatch.setenv(k, v)


def _flags(leaf_profiles=False, debug_rows=True):
    """debug_rows: the top-level f / b rows behind a record's fhash / bhash -- a first pass records them, a refinement pass does not"""
    from kalign_amd import api
    return (api.FLAG_DEBUG_ROWS if debug_rows else 0) | api.FLAG_DEVICE_GAPS | (api.FLAG_LEAF_PROFILES if leaf_profiles else 0)


def _same_records(got, want, tag, coded=None):
    """(rows) x 64 floats bit for bit; the first difference by column and field"""
    g, w = np.ascontiguousarray(got, np.float32).view(np.uint32).reshape(-1, 64), np.ascontiguousarray(want, np.float32).view(np.uint32).reshape(-1, 64)
    assert g.shape == w.shape, tag + ("rows", g.shape[0], w.shape[0])
    if not np.array_equal(g, w):
        col, field = (int(x) for x in np.argwhere(g != w)[0])
        code = int(coded[col]) if coded is not None and 0 < col < len(coded) - 1 else None
        raise AssertionError(tag + ("column %d of %d" % (col, g.shape[0]), "field %d" % field, "op code %s" % code,
                                    "got %r" % g.view(np.float32)[col, field], "want %r" % w.view(np.float32)[col, field],
                                    "%d floats differ" % int((g != w).sum())))


def _same_nodes(ctx, recs, paths, nodes, tag, task0=0, node_of=None):
    """every non-root node of a job's run against the recipe"""
    for t in range(len(nodes)):
        r = recs[task0 + t]
        c = r.c if node_of is None else node_of(t)
        _same_records(ctx.tree_profile(r.c, r.plen), nodes[c], tag + ("task %d" % t, "node %d" % c), paths[r.path_off:r.path_off + r.plen + 2])


def _same_leaves(ctx, leaves, tag, seq0=0):
    for i in sorted(leaves):
        _same_records(ctx.tree_profile(seq0 + i, len(leaves[i]) - 2), leaves[i], tag + ("sequence %d" % i,))
        ptr, plen = ctx.tree_profile_dev(seq0 + i)
        assert ptr and plen == len(leaves[i]) - 2, tag + (i,)


def _upload(ctx, j, leaf_profiles=False, n_anchors=0, debug_rows=True):
    codes, tasks, dist = mj.job(*j)
    subm, scal = mj.scoring(j)
    ctx.tree_upload(list(codes), tasks, subm, scal, dist, flags=_flags(leaf_profiles, debug_rows))
    if n_anchors:
        ctx.tree_build_consistency(n_anchors, 2.0)


def _modes(ctx, monkeypatch, j, leaf_profiles, n_anchors=0, modes=mj.MODES):
    want, (nodes, leaves) = mj.want(j, n_anchors), mj.expected(j, n_anchors)
    try:
        _upload(ctx, j, leaf_profiles, n_anchors)
        for mode in modes:
            _set(monkeypatch, mode)
            ctx.reload_env()
            tag = (mj.job_id(j), mode, "leaf records written" if leaf_profiles else "leaf records made in the merge")
            if j[0] != "ss":
                # the plan this mode runs: a profile task gets a cluster of at least two workgroups or, with KA_MAX_CLUSTER=1,
                # one (how many of them a task uses -- two from 320 rows on: the jobs of mj.BIG columns -- the kernel decides, and
                # the host does not see it).  A level of seq-seq tasks goes to the 128-register units: one workgroup per task.
                plan = ctx.debug_plan()
                mine = plan["blocks"][plan["blocks"][:, 0] == mj.target_task(j)]
                G = int(mine[0, 1]) >> 8
                assert plan["level_lean"].tolist() == [1] + [0] * (plan["levels"] - 1), tag + (plan["level_lean"],)
                assert (G == 1) if mode.get("KA_MAX_CLUSTER") == "1" else (G >= 2), tag + (G,)
                assert (mine[:, 1] >> 8 == G).all() and len(mine) >= G, tag + (mine,)
            ctx.tree_run()
            got = ctx.tree_download()
            # (the profiles first: a wrong record changes the tasks above it, and the first wrong node names the column and field)
            _same_nodes(ctx, got[0], got[1], nodes, tag)
            _same(got, want, tag, EXACT)
            assert ctx.fallback_runs() == 0, tag
            if leaf_profiles or j[3] in ("w1", "w025"):                 # (sequence weights: the merge reads the records, so they are written)
                _same_leaves(ctx, leaves, tag)
    finally:
        _set(monkeypatch, {})
        ctx.reload_env()


@pytest.mark.parametrize("j", JOBS, ids=mj.job_id)
def test_merged_profiles_in_every_form_of_the_merge(ctx, oracle, monkeypatch, j):
    """KA_FLAG_LEAF_PROFILES off: a sequence's records are made from its residue inside the merge"""
    _modes(ctx, monkeypatch, j, False)


@pytest.mark.parametrize("j", JOBS, ids=mj.job_id)
def test_merged_profiles_and_leaf_records_with_the_leaf_profiles_flag(ctx, oracle, monkeypatch, j):
    """KA_FLAG_LEAF_PROFILES on: the same merged profiles from records read in HBM, and every sequence's records read back are
    make_profile_n's for the penalties and score offset of the task that consumes it"""
    _modes(ctx, monkeypatch, j, True)


@pytest.mark.parametrize("j", PROFILE_JOBS, ids=mj.job_id)
def test_merged_profiles_in_default_mode(ctx, oracle, monkeypatch, j):
    """anchor consistency (three anchors): other kernels, other paths, the same merge"""
    _modes(ctx, monkeypatch, j, False, n_anchors=3, modes=[{}, {"KA_MERGE": "0"}, {"KA_MAX_CLUSTER": "1"}])


@pytest.mark.parametrize("j", JOBS, ids=mj.job_id)
def test_merged_profiles_after_refinement(ctx, oracle, j):
    """ka_tree_refine(1): paths in convert_raw_path's coding -- run open, extension, close, one-column runs, the terminal variants:
    the `code & 20` branch and ka_adj2; ka_tree_refine(3): three trials, first-pass coding.  A refinement pass writes the
    sequences' records: they are read back too."""
    _upload(ctx, j, debug_rows=False)
    for mode in (1, 3):
        want, (nodes, leaves) = mj.want(j, 0, mode), mj.expected(j, 0, mode)
        ctx.tree_refine(mode)
        recs, paths, gaps = ctx.tree_download()
        tag = (mj.job_id(j), "refine %d" % mode)
        _same_nodes(ctx, recs, paths, nodes, tag)
        for t, o in enumerate(want[0]):
            r = recs[t]
            for f in REFINED:
                assert getattr(r, f) == getattr(o, f), tag + (t, f, getattr(r, f), getattr(o, f))
            assert np.array_equal(paths[r.path_off:r.path_off + r.plen + 2], want[1][o.path_off:o.path_off + o.plen + 2]), tag + (t, "path")
        for i, g in enumerate(want[2]):
            assert np.array_equal(gaps[i], g), tag + (i, "gaps")
        _same_leaves(ctx, leaves, tag)


def _levels(tasks, n):
    lvl = {}
    for a, b, c in np.asarray(tasks).tolist():
        lvl[c] = 1 + max(lvl.get(a, -1), lvl.get(b, -1))
    return lvl


def _forest(ctx, monkeypatch, alphabet, leaf_profiles):
    """every job of one alphabet and one scoring (the plain tables), copied until the widest level with profile tasks holds more
    than 300 of them -- more than the GPU has CUs, and not only seq-seq tasks: that level goes to the 4-wave kind of launch, the
    seq-seq level below it to the 128-register units (the rule of tests/test_gpu_strip_edges.py's forests).  Every copy's
    profiles must equal the recipe of its job alone, in two runs on one upload."""
    from kalign_amd import guide
    mine = [j for j in JOBS if j[2] == alphabet and j[3] == "plain"]
    per_level = {}
    for j in mine:
        codes, tasks, _ = mj.job(*j)
        for (a, b, c), l in zip(tasks.tolist(), _levels(tasks, len(codes)).values()):
            if a >= len(codes) or b >= len(codes):
                per_level[l] = per_level.get(l, 0) + 1
    widest = max(per_level, key=lambda l: per_level[l])
    copies = 300 // per_level[widest] + 1
    jobs = [(list(codes), tasks, dist) for codes, tasks, dist in (mj.job(*j) for j in mine)] * copies
    fc, ft, fd, spans = guide.forest(jobs)
    assert per_level[widest] * copies > 300
    subm, scal = mj.scoring(mine[0])
    try:
        ctx.tree_upload(fc, ft, subm, scal, fd, flags=_flags(leaf_profiles))
        for run in ("run 1", "run 2"):
            _set(monkeypatch, {})
            ctx.reload_env()
            # the seq-seq level: lean (1); the widest profile level: the 4-wave kind (2); it is a launch of its own, neither
            # queued nor chained.  Above it the levels are
            # narrower than the device (the targets of the 1 / 3 and 3 / 2 jobs, the roots): 8-wave tasks, chained into one launch
            plan = ctx.debug_plan()
            assert widest == 1 and plan["levels"] == 4 and plan["level_lean"].tolist() == [1, 2, 0, 0], (alphabet, run, plan["level_lean"])
            assert plan["queue_first"] == -1 and plan["chain_level"] == 2, (alphabet, run, plan["queue_first"], plan["chain_level"])
            ctx.tree_run()
            got = ctx.tree_download()
            assert ctx.fallback_runs() == 0, (alphabet, run)
            assert (len(got[2]), len(got[0])) == (len(fc), len(ft)) == tuple(sum(s[i] for s in spans) for i in (2, 3)), (alphabet, run)
            for k, (s0, t0, ns, nt) in enumerate(spans):
                j = mine[k % len(mine)]
                tag = (mj.job_id(j), run, "copy %d" % (k // len(mine)))
                nodes, leaves = mj.expected(j)
                _same_nodes(ctx, got[0], got[1], nodes, tag, t0, lambda t, ns=ns: ns + t)
                _same(got, mj.want(j), tag, FOREST, t0, s0, (ns, nt))
                if leaf_profiles:
                    _same_leaves(ctx, leaves, tag, s0)
    finally:
        _set(monkeypatch, {})
        ctx.reload_env()


@pytest.mark.parametrize("alphabet,leaf_profiles", [("protein", False), ("dna", True), ("bzx", False)])
def test_forest_of_merge_jobs(ctx, oracle, monkeypatch, alphabet, leaf_profiles):
    """the 4-wave kernel and the lean units' merge (KA_MERGE_LEAN)"""
    _forest(ctx, monkeypatch, alphabet, leaf_profiles)


# ---- reading a sequence's records back ---------------------------------------------------------------------------------------

def _refused(ctx, node, word, host=True):
    """ka_tree_get_profile (host: it wants a finished run first) and ka_tree_profile_dev"""
    from kalign_amd.api import KalignAmdError
    for read in ([lambda: ctx.tree_profile(node, 400)] if host else []) + [lambda: ctx.tree_profile_dev(node)]:
        with pytest.raises(KalignAmdError, match=word):
            read()


def test_leaf_read_fails_without_the_flag(ctx, oracle):
    """no flag, no sequence weights, a first pass: nothing wrote the records -- an error that names the flag, not arena memory"""
    j = ("ps", 33, "protein", "plain")
    _upload(ctx, j)
    ctx.tree_run()
    recs, paths, _ = ctx.tree_download()
    for i in range(len(mj.job(*j)[0])):
        _refused(ctx, i, "KA_FLAG_LEAF_PROFILES")
    _same_nodes(ctx, recs, paths, mj.expected(j)[0], (mj.job_id(j),))       # (a node's profile is read as before)
    # a refinement pass writes them; the first pass after it does not
    ctx.tree_refine(1)
    ctx.tree_sync()
    _same_leaves(ctx, mj.expected(j, 0, 1)[1], (mj.job_id(j), "refined"))
    ctx.tree_run()
    ctx.tree_sync()
    _refused(ctx, 0, "KA_FLAG_LEAF_PROFILES")


@pytest.mark.parametrize("again", ["upload", "reset"])
def test_leaf_read_fails_after_a_partial_first_pass_that_follows_a_refinement(ctx, oracle, again):
    """what counts is the launch that ran the consuming task, not the context's last ka_tree_refine: a new upload or a reset,
    then ka_tree_run_tasks -- a first pass, which writes no leaf records without the flag -- leaves only stale arena memory"""
    j = ("ps", 33, "protein", "plain")
    _upload(ctx, j)
    ctx.tree_refine(1)
    ctx.tree_sync()
    _same_leaves(ctx, mj.expected(j, 0, 1)[1], (mj.job_id(j), "refined"))
    if again == "upload":
        j = ("sp", 32, "protein", "plain")
        _upload(ctx, j)
    else:
        ctx.tree_reset()
    n = len(mj.job(*j)[0])
    ctx.tree_run_tasks(list(range(n - 1)))
    recs, paths = ctx.tree_download_tasks(list(range(n - 1)))
    for i in range(n):
        _refused(ctx, i, "KA_FLAG_LEAF_PROFILES")
    nodes = mj.expected(j)[0]
    for t, r in enumerate(recs[:-1]):
        _same_records(ctx.tree_profile(r.c, r.plen), nodes[r.c], (mj.job_id(j), again, "node %d" % r.c), paths[r.path_off:r.path_off + r.plen + 2])


def test_leaf_read_with_sequence_weights_needs_no_flag(ctx, oracle):
    j = ("ps", 32, "dna", "w1")
    _upload(ctx, j)
    ctx.tree_run()
    ctx.tree_sync()
    _same_leaves(ctx, mj.expected(j)[1], (mj.job_id(j),))


def test_leaf_read_fails_before_its_task_has_run(ctx, oracle):
    """the flag is set, but a sequence's records carry the penalties of the task that consumes it: not there before that task"""
    j = ("ps", 33, "bzx", "scaled")                                      # tasks (0, 1), (4, 2), (5, 3)
    _upload(ctx, j, leaf_profiles=True)
    _refused(ctx, 0, "has not run", host=False)
    ctx.tree_run_tasks([0])
    ctx.tree_sync()
    leaves = mj.expected(j)[1]
    _same_leaves(ctx, {i: leaves[i] for i in (0, 1)}, (mj.job_id(j), "task 0"))
    _refused(ctx, 2, "has not run")
    _refused(ctx, 3, "has not run")
    ctx.tree_run_tasks([1, 2])
    ctx.tree_sync()
    _same_leaves(ctx, leaves, (mj.job_id(j), "all tasks"))
    assert ctx.L.ka_abi_version() >= 21
