"""The gathered profile-profile dot product (ka_pass.h: KA_SPARSE_NT) against the oracle bit for bit, and against the dense form of
the same kernel (KA_SPARSE=0) byte for byte.

The gathered form is built into the two-row strip of the 4-wave fast-mode kernel, which serves levels with more tasks than the
device has CUs: the designed jobs of tests/sparse_jobs.py run as forests whose root level is that wide (the rule of
tests/test_gpu_forest.py and of the forests in tests/test_gpu_strip_edges.py).  tests/test_sparse_strip_inputs.py proves on the host
what the jobs are: row profiles of two sequences whose strips all stay within the bound (a lone partial strip of 35 rows with an
odd last row, 75-row strips, a full 128-row strip handing over to a partial one, the 23-residue alphabet, windows with fewer columns
than a strip has lanes), and row profiles with designed columns of exactly NT and exactly NT + 1 distinct residues, so that one strip
of a pass runs gathered and its neighbour dense.  Every copy of every job must come out as the oracle's answer for that job alone --
record (with the hashes of the top-level f / b rows), coded path, gap arrays -- in two runs per switch on one upload.

That the gathered form is what ran is read from the breadcrumbs of a context made with KA_TRACE=1: a strip of a kernel built with
the form leaves a mark for the form it chose.

Not here: a row with no residue at all (a merged profile has none: tests/test_sparse_strip_inputs.py asserts it for every profile of
every job; the shortest list a job can make is the single row of a lane whose row B lies below the strip's last row -- rows70), and
the one-row-per-lane strip of the helper-wave kernel, which runs dense."""
import numpy as np
import pytest

import sparse_jobs as sp
import strip_jobs as sj
from test_gpu_parity import EXACT

pytestmark = pytest.mark.gpu

FOREST = [f for f in EXACT if f not in ("a", "b", "c")]              # (a forest renumbers a job's nodes)
WIDE = 300                                                           # more root tasks than the device has CUs


@pytest.fixture(scope="module")
def ctx():
    import kalign_amd
    c = kalign_amd.Context(0)
    yield c
    c.close()


def _set(monkeypatch, ctx, sparse):
    monkeypatch.delenv("KA_SPARSE", raising=False)
    if sparse is not None:
        monkeypatch.setenv("KA_SPARSE", sparse)
    ctx.reload_env()


def _check(got, names, spans, tag):
    recs, paths, gaps = got
    for j, (s0, t0, ns, nt) in enumerate(spans):
        name = names[j % len(names)]
        orecs, opaths, ogaps, _ = sp.want(name)
        assert (ns, nt) == (len(ogaps), len(orecs)), tag + (name,)
        for t, o in enumerate(orecs):
            r = recs[t0 + t]
            for f in FOREST:
                assert getattr(r, f) == getattr(o, f), tag + (name, j, t, f, getattr(r, f), getattr(o, f))
            assert np.array_equal(paths[r.path_off:r.path_off + r.plen + 2], opaths[o.path_off:o.path_off + o.plen + 2]), tag + (name, j, t, "path")
        for i, g in enumerate(ogaps):
            assert np.array_equal(gaps[s0 + i], g), tag + (name, j, i, "gaps")


def _bytes(got):
    """a run's output as bytes, whatever place a run gave a task's path in the path arena: every field of every record but
    path_off, every coded path, every gap array"""
    recs, paths, gaps = got
    fields = [f for f, _ in type(recs[0])._fields_ if f != "path_off"]
    bits = lambda v: np.float32(v).tobytes() if isinstance(v, float) else v        # (a float by its bits)
    return ([tuple(bits(getattr(r, f)) for f in fields) for r in recs],
            [paths[r.path_off:r.path_off + r.plen + 2].tobytes() for r in recs], [np.asarray(g).tobytes() for g in gaps])


def _forest(ctx, monkeypatch, names):
    from kalign_amd import api, guide
    copies = WIDE // len(names) + 1
    jobs = [sp.job(n) for n in names] * copies
    fc, ft, fd, spans = guide.forest([(list(c), t, d) for c, t, d in jobs])
    subm, scal = sj.scoring("protein")
    seen = {}
    try:
        ctx.tree_upload(fc, ft, subm, scal, fd, flags=api.FLAG_DEBUG_ROWS | api.FLAG_DEVICE_GAPS)
        for sparse in ("1", "0", None):
            _set(monkeypatch, ctx, sparse)
            # the roots' level is wider than the device and holds profile tasks: a launch of the 4-wave kind (2)
            plan = ctx.debug_plan()
            assert plan["level_lean"][plan["levels"] - 1] == 2, (names, sparse, plan["level_lean"])
            for run in ("run 1", "run 2"):
                ctx.tree_run()
                got = ctx.tree_download()
                assert ctx.fallback_runs() == 0, (names, sparse, run)
                assert (len(got[2]), len(got[0])) == (len(fc), len(ft)), (names, sparse, run)
                _check(got, names, spans, (sparse, run))
                seen[(sparse, run)] = _bytes(got)
        first = seen[("1", "run 1")]
        for key, val in seen.items():
            assert val == first, ("KA_SPARSE=%s, %s: not the bytes of KA_SPARSE=1, run 1" % key)
    finally:
        _set(monkeypatch, ctx, None)


GATHERED, DENSE = 60, 61                                             # KA_TRACE_GATHERED, KA_TRACE_DENSE (ka_shared.h)


@pytest.mark.parametrize("names,sparse,want", [(sp.pair_names(), None, (1, -1)), (sp.bound_names(), None, (1, 1)),
                                               (sp.pair_names(), "0", (-1, 1))], ids=["pair", "bound", "pair-KA_SPARSE=0"])
def test_the_form_that_ran(oracle, monkeypatch, names, sparse, want):
    """pair jobs: every strip of the 4-wave kernel gathered, none dense; the bound job: both; KA_SPARSE=0: none gathered"""
    import kalign_amd
    from kalign_amd import guide
    monkeypatch.setenv("KA_TRACE", "1")
    monkeypatch.delenv("KA_SPARSE", raising=False)
    if sparse is not None:
        monkeypatch.setenv("KA_SPARSE", sparse)
    c = kalign_amd.Context(0)
    try:
        jobs = [sp.job(n) for n in names] * (WIDE // len(names) + 1)
        fc, ft, fd, _ = guide.forest([(list(x), t, d) for x, t, d in jobs])
        subm, scal = sj.scoring("protein")
        c.tree_upload(fc, ft, subm, scal, fd)
        plan = c.debug_plan()
        assert plan["level_lean"][plan["levels"] - 1] == 2, plan["level_lean"]
        c.tree_run()
        c.tree_sync()
        tr = c.debug_trace()
        assert (int(tr[GATHERED]), int(tr[DENSE])) == want, tr[56:64]
    finally:
        c.close()


def test_strips_within_the_bound(ctx, oracle, monkeypatch):
    """nsip 2 + 2: partial strips, a full strip handing over to a partial one, B / Z / X, fewer columns than lanes"""
    _forest(ctx, monkeypatch, sp.pair_names())


def test_neighbouring_strips_either_side_of_the_bound(ctx, oracle, monkeypatch):
    """exactly NT and exactly NT + 1 distinct residues in neighbouring strips of one pass"""
    _forest(ctx, monkeypatch, sp.bound_names())
