"""The strip passes at their row and column edges, against the oracle bit for bit: ka_strip (128-row strips and, with KA_Q1, 64-row
ones; hand-over through the HBM row buffer, through the LDS ring and between the workgroups of a cluster), ka_wstrip / ka_whelper
(strips with helper waves), ka_packed and ka_strip's small and empty passes (KA_SUBTREE=0), and -- as forests -- the 4-wave kernel's
strips.

The jobs are tests/strip_jobs.py's: small tasks whose root has exactly the rows and columns that put a pass on an edge -- strips of
1, 2, 63, 64, 65, 127 and 128 rows as the only, the second and the third strip of a pass, the empty pass, column counts either side of
a 64-column hand-over batch and of the 128-column wrap of the column ring, more columns than the LDS ring has slots, and tasks on two
workgroups.  tests/test_strip_edge_inputs.py proves on the host that they are.  Every mode runs twice on one upload: the second run
meets the hand-over control words and progress words the first one left.  Compared per task: the record (kind, swap, meetup, score,
the hashes of the top-level f / b rows -- the value that shows a wrong hand-over even where the argmax survives it), the coded path;
per sequence: the gap array."""
import numpy as np
import pytest

import strip_jobs as sj
from test_gpu_parity import EXACT

pytestmark = pytest.mark.gpu

FOREST = [f for f in EXACT if f not in ("a", "b", "c")]              # (a forest renumbers a job's nodes)


@pytest.fixture(scope="module")
def ctx():
    import kalign_amd
    c = kalign_amd.Context(0)
    yield c
    c.close()


def _same(got, want, tag, fields=EXACT, task0=0, seq0=0, span=None):
    """the tasks [task0 ..) and sequences [seq0 ..) of a run against a job's oracle answer; span: the (sequences, tasks) the job
    has in a forest (None: the run is this job alone) -- neither fewer nor more than the oracle's"""
    recs, paths, gaps = got
    orecs, opaths, ogaps = want
    if span is None:
        span = (len(gaps), len(recs))
    assert span == (len(ogaps), len(orecs)), tag + ("sequences, tasks", span)
    for t, o in enumerate(orecs):
        r = recs[task0 + t]
        for f in fields:
            assert getattr(r, f) == getattr(o, f), tag + (t, f, getattr(r, f), getattr(o, f))
        assert np.array_equal(paths[r.path_off:r.path_off + r.plen + 2], opaths[o.path_off:o.path_off + o.plen + 2]), tag + (t, "path")
    for i, g in enumerate(ogaps):
        assert np.array_equal(gaps[seq0 + i], g), tag + (i, "gaps")


def _set(monkeypatch, mode):
    for k in sj.MODE_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in mode.items():
        monkeypatch.setenv(k, v)


def _modes(ctx, monkeypatch, case, modes, n_anchors=0):
    from kalign_amd import api
    codes, tasks, dist = sj.job(*case)
    subm, scal = sj.scoring(case[3])
    want = sj.want(*case, n_anchors)
    try:
        ctx.tree_upload(list(codes), tasks, subm, scal, dist, flags=api.FLAG_DEBUG_ROWS | api.FLAG_DEVICE_GAPS)
        if n_anchors:
            ctx.tree_build_consistency(n_anchors, 2.0)
        for mode in modes:
            _set(monkeypatch, mode)
            ctx.reload_env()
            if case[0] != "ss":
                # the plan this mode runs: the root's level is a launch of the 8-wave kind (ka_strip / ka_wstrip with the LDS
                # hand-over and helper waves, which the kernel chooses per level), on a cluster of at least two workgroups or,
                # with KA_MAX_CLUSTER=1, on one.  This pins the cluster the planner gives a lone task, whatever its rows: how
                # many of its workgroups the task uses (two from 320 rows on: the hand-over between workgroups) the kernel
                # decides, and the host does not see it
                plan = ctx.debug_plan()
                mine = plan["blocks"][plan["blocks"][:, 0] == len(tasks) - 1]
                assert plan["level_lean"][plan["levels"] - 1] == 0, (case, mode, plan["level_lean"])
                assert (len(mine) == 1) if mode.get("KA_MAX_CLUSTER") == "1" else (len(mine) >= 2), (case, mode, len(mine))
                assert (mine[:, 1] >> 8 == len(mine)).all(), (case, mode, mine)
            for run in (1, 2):
                ctx.tree_run()
                _same(ctx.tree_download(), want, (sj.case_id(case), mode, "run %d" % run))
                assert ctx.fallback_runs() == 0, (case, mode, run)
    finally:
        _set(monkeypatch, {})
        ctx.reload_env()


@pytest.mark.parametrize("case", sj.cases(), ids=sj.case_id)
def test_strip_edges(ctx, oracle, monkeypatch, case):
    _modes(ctx, monkeypatch, case, sj.MODES)


@pytest.mark.parametrize("case", sj.cons_cases(), ids=sj.case_id)
def test_strip_edges_with_anchor_consistency(ctx, oracle, monkeypatch, case):
    """the reference's default mode: the NB instances of the strips (bonus terms in every cell)"""
    _modes(ctx, monkeypatch, case, sj.CONS_MODES, n_anchors=3)


def _forest(ctx, monkeypatch, alphabet):
    """every profile job of one alphabet, copied until the widest level with profile tasks holds at least 300 of them -- more than
    the GPU has CUs, and not only seq-seq tasks: the level goes to the 4-wave kind of launch (the rule of tests/test_gpu_forest.py).
    Every copy of every job must come out as the oracle's answer for that job alone, in two runs on one upload."""
    from kalign_amd import api, guide
    cases = [c for c in sj.cases() if c[0] != "ss" and c[3] == alphabet]
    copies = 300 // len(cases) + 1                                    # (each job's only profile task of the widest level is its root)
    jobs = [(list(codes), tasks, dist) for codes, tasks, dist in (sj.job(*c) for c in cases)] * copies
    fc, ft, fd, spans = guide.forest(jobs)
    assert len(cases) * copies >= 300
    subm, scal = sj.scoring(alphabet)
    try:
        ctx.tree_upload(fc, ft, subm, scal, fd, flags=api.FLAG_DEBUG_ROWS | api.FLAG_DEVICE_GAPS)
        for run in ("run 1", "run 2"):
            _set(monkeypatch, {})
            ctx.reload_env()
            # the roots' level is wider than the device and not all seq-seq: a launch of the 4-wave kind (2)
            plan = ctx.debug_plan()
            assert plan["levels"] == 2 and plan["level_lean"].tolist() == [1, 2], (alphabet, run, plan["level_lean"])
            assert plan["chain_level"] == -1 and plan["queue_first"] == -1, (alphabet, run)
            ctx.tree_run()
            got = ctx.tree_download()
            assert ctx.fallback_runs() == 0, (alphabet, run)
            assert (len(got[2]), len(got[0])) == (len(fc), len(ft)) == tuple(sum(s[i] for s in spans) for i in (2, 3)), (alphabet, run)
            for j, (s0, t0, ns, nt) in enumerate(spans):
                case = cases[j % len(cases)]
                _same(got, sj.want(*case), (sj.case_id(case), run, "copy %d" % (j // len(cases))), FOREST, t0, s0, (ns, nt))
    finally:
        _set(monkeypatch, {})
        ctx.reload_env()


@pytest.mark.parametrize("alphabet", ["protein", "dna"])
def test_forest_of_strip_edges(ctx, oracle, monkeypatch, alphabet):
    """the 4-wave kernel's strips"""
    _forest(ctx, monkeypatch, alphabet)


def test_forest_of_strip_edges_with_b_z_x(ctx, oracle, monkeypatch):
    """23 residue classes: the 4-wave kernel's NRES = 23 instance"""
    _forest(ctx, monkeypatch, "bzx")
