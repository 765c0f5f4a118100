"""The streamed-bonus kernels (`--consistency K`, 5 < K <= 128: units 6 - 9, picked by ka_cons_big()) at their edges, against
the oracle bit for bit.

With more than five anchors a DP row's bonus entries are not held in registers but walked: KaBonus<NB>::STREAM (ka_pass.h)
keeps the entry a lane meets next and advances along the row's sorted list, forward or backward; ka_cons_entries' streamed
branch (ka_profile.h) collects, sums, sorts and closes that list in a K-sized slice of the task's scratch.  None of this
runs in the default mode.  The jobs (tests/stream_jobs.py) put the lists' ends where the walk can go wrong -- rows without
entries, rows whose list the wrap-around entry joins, summed cells, lists of 25 entries at 128 anchors -- and the DP
windows' edges where the subtree engine reloads a lane's stream per slot (tests/test_gpu_subtree_step.py's shapes);
tests/test_stream_bonus_inputs.py checks on the host that they do.  The oracle's restatement for more than five anchors is
pinned to the real reference by the cons_stream_* / refine_cons_stream_* goldens (tests/test_oracle_golden.py).

Every case first asserts that the job really has more than five anchors: it cannot pass on the K <= 5 kernels."""
import functools
import os

import numpy as np
import pytest

import stream_jobs as sj

pytestmark = pytest.mark.gpu

EXACT = ["plen", "kind", "swapped", "meet", "transition", "score"]
HASHES = ["fhash", "bhash"]                         # (uploads with FLAG_DEBUG_ROWS)


@functools.lru_cache(maxsize=None)
def _job(kind, *args):
    return getattr(sj, kind + "_job")(*args)


@functools.lru_cache(maxsize=None)
def _want(k, kind, *args):
    """the oracle's answer for a job, computed once: (recs, paths, gaps, anchor ids, maps, bonus hashes)"""
    from oracle import oracledrv
    codes, tasks, dist, dna = _job(kind, *args)
    subm, scal = sj.scoring(dna)
    return oracledrv.msa_tree_cons(codes, tasks, subm, scal, dist, k, 2.0)


def _same_table(ctx, want, tag):
    ids, maps = ctx.tree_consistency()
    assert len(ids) > 5, (tag, len(ids))                           # the streamed set, not its K <= 5 sibling
    assert np.array_equal(ids, want[3]), tag
    for i, (ra, rb) in enumerate(zip(maps, want[4])):
        for k, (a, b) in enumerate(zip(ra, rb)):
            assert np.array_equal(a, b), (tag, i, k)


def _same_alignment(got, want, tag, fields=EXACT):
    recs, paths, gaps = got
    orecs, opaths, ogaps = want[:3]
    assert len(recs) == len(orecs)
    for t, (r, o) in enumerate(zip(recs, orecs)):
        for f in fields:
            assert getattr(r, f) == getattr(o, f), (tag, t, f, getattr(r, f), getattr(o, f))
        assert np.array_equal(paths[r.path_off:r.path_off + r.plen + 2], opaths[o.path_off:o.path_off + o.plen + 2]), (tag, t)
    for i, (a, b) in enumerate(zip(gaps, ogaps)):
        assert np.array_equal(a, b), (tag, i)


def _same_profiles(ctx, oracle, recs, want, tag):
    L = oracle.lib()
    for t, (r, o) in enumerate(zip(recs[:-1], want[0])):
        prof = ctx.tree_profile(r.c, r.plen)
        assert L.ko_fnv1a(prof.ctypes.data, 4 * 64 * (r.plen + 2)) == o.prof_hash, (tag, t)


def _run(oracle, k, kind, *args, twice=False):
    """one context per case: the job in default mode with k anchors, everything compared with the oracle"""
    import kalign_amd
    from kalign_amd import api
    tag = (kind,) + args + (k,)
    codes, tasks, dist, dna = _job(kind, *args)
    subm, scal = sj.scoring(dna)
    want = _want(k, kind, *args)
    ctx = kalign_amd.Context(0)
    try:
        got = ctx.msa_tree(codes, tasks, subm, scal, dist, flags=api.FLAG_DEBUG_ROWS, n_anchors=k, weight=2.0)
        _same_table(ctx, want, tag)
        _same_alignment(got, want, tag, EXACT + HASHES)
        _same_profiles(ctx, oracle, got[0], want, tag)
        if twice:                                                  # the arena has grown and the residue -> column table is reset
            ctx.tree_run()
            _same_alignment(ctx.tree_download(), want, tag + ("second run",), EXACT + HASHES)
        assert ctx.fallback_runs() == 0, tag
    finally:
        ctx.close()


@pytest.mark.parametrize("la,lb", sj.SHAPES)
@pytest.mark.parametrize("k", [8, 128])
@pytest.mark.parametrize("dna", [False, True])
def test_window_edges_with_eight_anchors(oracle, la, lb, k, dna):
    """8 sequences, all of them anchors (asked for as 8 and as 128: the cap): the odd one in a seq-seq task, in a seq-profile task
    and in a profile-profile task; windows of 1 - 64 rows (subtrees), strips of 65 / 128 / 129 rows, windows of 1 - 3 columns"""
    _run(oracle, k, "shape", la, lb, dna)


@pytest.mark.parametrize("k", sj.BOUNDARY_K)
def test_anchor_count_boundaries(oracle, k):
    """the votes take five anchors per sweep: one more than one sweep, two sweeps and one more, several; rows with more than
    five entries in every job"""
    _run(oracle, k, "boundary", k)


@pytest.mark.parametrize("dna", [True, False], ids=["nt", "aa"])
def test_128_anchors_and_a_second_run(oracle, dna):
    """130 sequences, 128 anchors: the longest lists the scratch slice has to hold (K + the wrap-around entry + sentinels within
    KA_NB_BIG), the arena grown for K-sized tables; then the same context runs the tree again"""
    _run(oracle, 128, "k128", dna, twice=True)


def test_a_context_keeps_its_arena_from_table_to_table(oracle):
    """ka_tree_build_consistency grows the scratch arena for the K-sized slices -- from what the uploaded job's plan asked for.  (It
    used to multiply what the context HELD: a context that served one job with more than five anchors after the other grew its arena
    by the same factor every time, until hipMalloc failed; tests/test_gpu_refine.py's shared context met that on the cons_stream_*
    goldens.)  The same two jobs in turn on one context: the arena is the larger job's from its first table on, answers are the oracle's;
    then arenas that start too small (KA_DEBUG_SMALL_ARENAS): overflow, growth, a second run, the same answer."""
    import kalign_amd
    from kalign_amd import api
    ctx = kalign_amd.Context(0)
    try:
        assert ctx.L.ka_abi_version() >= 16                        # (ka_ctx_arena_bytes)
        sizes = []
        for k in (33, 11, 33, 11, 33):
            codes, tasks, dist, dna = _job("boundary", k)
            subm, scal = sj.scoring(dna)
            got = ctx.msa_tree(codes, tasks, subm, scal, dist, n_anchors=k, weight=2.0)
            sizes.append(ctx.arena_bytes())
            _same_table(ctx, _want(k, "boundary", k), ("arena", k))
            _same_alignment(got, _want(k, "boundary", k), ("arena", k))
        assert sizes[0] > 0 and sizes[2:] == [max(sizes[:2])] * 3, sizes
        assert ctx.fallback_runs() == 0
        ctx.debug_set_hooks(1)                                     # KA_DEBUG_SMALL_ARENAS
        codes, tasks, dist, dna = _job("boundary", 11)
        subm, scal = sj.scoring(dna)
        ctx.tree_upload(codes, tasks, subm, scal, dist, flags=api.FLAG_DEVICE_GAPS)
        ctx.debug_set_hooks(0)
        ctx.tree_build_consistency(11, 2.0)
        small = ctx.arena_bytes()
        assert small < min(sizes), (small, sizes)                  # (the table's growth starts from the small arena, not from the plan's)
        _same_table(ctx, _want(11, "boundary", 11), ("small arenas", 11))
        ctx.tree_run()
        got = ctx.tree_download()
        assert ctx.arena_bytes() > small                           # it overflowed, grew, and the run was repeated
        _same_alignment(got, _want(11, "boundary", 11), ("small arenas", 11))
        assert ctx.fallback_runs() == 0
    finally:
        ctx.close()


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_refinement_with_eleven_anchors(oracle, mode):
    """unit 9 (ka_refine_kernel_cons_big): all edges, the edges at or below the median confidence, inline trials"""
    import kalign_amd
    codes, tasks, dist, dna = _job("refine")
    subm, scal = sj.scoring(dna)
    first = _want(11, "refine")
    conf = np.array([r.confidence for r in first[0]], np.float32)
    orecs, opaths, ogaps = oracle.msa_tree_refine(codes, tasks, subm, scal, dist, mode=mode, conf_in=conf, n_anchors=11, weight=2.0)
    ctx = kalign_amd.Context(0)
    try:
        ctx.tree_upload(codes, tasks, subm, scal, dist)
        ctx.tree_build_consistency(11, 2.0)
        _same_table(ctx, first, ("refine", mode))
        if mode != 3:
            ctx.tree_run()
            _same_alignment(ctx.tree_download(), first, ("refine", mode, "first pass"))
        ctx.tree_refine(mode, conf)
        recs, paths, gaps = ctx.tree_download()
        for t, (r, o) in enumerate(zip(recs, orecs)):
            assert r.plen == o.plen and r.confidence == o.confidence, (mode, t)
            assert np.array_equal(paths[r.path_off:r.path_off + r.plen + 2], opaths[o.path_off:o.path_off + o.plen + 2]), (mode, t)
        for a, b in zip(gaps, ogaps):
            assert np.array_equal(a, b), mode
        if mode == 1:
            assert any(not np.array_equal(a, b) for a, b in zip(ogaps, first[2]))          # (the refinement changed something)
        assert ctx.fallback_runs() == 0
    finally:
        ctx.close()


def test_forest_of_two_alignments_with_eight_anchors(oracle):
    """two different families as one forest job: each tree selects eight anchors among its own sequences"""
    import kalign_amd
    from kalign_amd import guide
    jobs = [_job("shape", 65, 63, False), _job("shape", 3, 64, False)]
    wants = [_want(8, "shape", 65, 63, False), _want(8, "shape", 3, 64, False)]
    subm, scal = sj.scoring(False)
    codes, tasks, dist, spans = guide.forest([(j[0], j[1], j[2]) for j in jobs])
    ctx = kalign_amd.Context(0)
    try:
        recs, paths, gaps = ctx.msa_tree(codes, tasks, subm, scal, dist, n_anchors=8, weight=2.0)
        ids, maps = ctx.tree_consistency()
        assert len(ids) == 16 and np.array_equal(ids, np.concatenate([w[3] + s[0] for w, s in zip(wants, spans)]))
        for w, (s0, t0, ns, nt) in zip(wants, spans):
            _same_alignment((recs[t0:t0 + nt], paths, gaps[s0:s0 + ns]), w, ("forest", s0))
            for ra, rb in zip(maps[s0:s0 + ns], w[4]):
                for a, b in zip(ra, rb):
                    assert np.array_equal(a, b)
        assert ctx.fallback_runs() == 0
    finally:
        ctx.close()


def test_table_built_in_two_parts(oracle):
    """ka_tree_build_consistency_part at K = 11: two contexts build a share of the N x K maps each, the shares are exchanged
    device to device, and both contexts align the tree on the assembled table"""
    import torch
    import kalign_amd
    torch.cuda.init()
    codes, tasks, dist, dna = _job("boundary", 11)
    subm, scal = sj.scoring(dna)
    want = _want(11, "boundary", 11)
    ctxs = [kalign_amd.Context(0) for _ in range(2)]
    try:
        for r, c in enumerate(ctxs):
            c.tree_upload(codes, tasks, subm, scal, dist)
            c.tree_build_consistency_part(11, 2.0, r, 2)
        tables = [c.cons_table() for c in ctxs]
        for r in range(2):
            lo, hi = ctxs[r].cons_part_range(r, 2)
            assert ctxs[1 - r].cons_part_range(r, 2) == (lo, hi) and hi > lo
            tables[1 - r][lo:hi].copy_(tables[r][lo:hi])
        torch.cuda.synchronize()
        flat = np.concatenate([np.asarray(m, np.int32) for row in want[4] for m in row])
        for r, c in enumerate(ctxs):
            assert np.array_equal(tables[r].cpu().numpy(), flat), r
            _same_table(c, want, ("parts", r))
            c.tree_run()
            _same_alignment(c.tree_download(), want, ("parts", r))
            assert c.fallback_runs() == 0
    finally:
        for c in ctxs:
            c.close()


@pytest.mark.parametrize("k", [11, 33])
def test_randomised_schedules_give_the_oracle_answer(oracle, k, monkeypatch):
    """tests/test_gpu_stress.py's switches over a K = 11 and a K = 33 job: who computes when varies, the answer does not"""
    import kalign_amd
    from kalign_amd import api
    from test_gpu_stress import SWITCHES
    reps = int(os.environ.get("KA_STRESS_REPS", "20"))
    codes, tasks, dist, dna = _job("boundary", k)
    subm, scal = sj.scoring(dna)
    want = _want(k, "boundary", k)
    rng = np.random.RandomState(4000 + k)
    ctx = kalign_amd.Context(0)
    try:
        ctx.tree_upload(codes, tasks, subm, scal, dist, flags=api.FLAG_DEBUG_ROWS | api.FLAG_DEVICE_GAPS)
        ctx.tree_build_consistency(k, 2.0)
        _same_table(ctx, want, ("stress", k))
        for rep in range(reps):
            chosen = {}
            for name, vals in SWITCHES.items():
                v = vals[rng.randint(len(vals))]
                if v is None:
                    monkeypatch.delenv(name, raising=False)
                else:
                    monkeypatch.setenv(name, v)
                    chosen[name] = v
            rng.randint(3)                  # the draw of a retired switch (it was the last key, three values): every repetition keeps the settings it always had
            ctx.reload_env()
            ctx.tree_run()
            _same_alignment(ctx.tree_download(), want, ("stress", k, rep, tuple(sorted(chosen.items()))), EXACT + HASHES)
            assert ctx.fallback_runs() == 0, (k, rep, chosen)
    finally:
        for name in SWITCHES:
            monkeypatch.delenv(name, raising=False)
        ctx.close()
