"""Host-only: the seeded jobs of tests/test_gpu_merge.py (tests/merge_jobs.py) are what they are listed for, and the recipe
that test compares the device's records with is the oracle's -- and the real reference's -- merged profile.

Conditions on the INPUTS, measured with the oracle: a later change of seeds or of the generator cannot quietly move that suite
off the op codes, the run lengths and the item-walk edges it is there for."""
import ctypes as C
import itertools

import numpy as np
import pytest

import merge_jobs as mj
from util import Golden

JOBS = mj.jobs()
PLANNED = [j for j in JOBS if j[1] > 4]               # (two sequences of one and two letters have no room for planned edits)
PROFILE_JOBS = [j for j in JOBS if j[0] != "ss"]


def _hash(oracle, prof):
    p = np.ascontiguousarray(prof, np.float32)
    return oracle.lib().ko_fnv1a(p.ctypes.data, p.nbytes)


def _path(recs, paths, t):
    r = recs[t]
    return paths[r.path_off:r.path_off + r.plen + 2]


def _target_path(j, refine=0):
    recs, paths, _ = mj.want(j, 0, refine)
    return _path(recs, paths, mj.target_task(j))


def _nonroot_paths(j, refine=0):
    recs, paths, _ = mj.want(j, 0, refine)
    return [_path(recs, paths, t) for t in range(len(recs) - 1)]


def test_the_table_is_the_issue_of_record():
    assert len(JOBS) == len(set(JOBS)) == 4 * 9 + 3 + 4 + 3 + 2 + 4
    assert {j[0] for j in JOBS if j[1] == mj.BIG} == {"ps", "sp", "pp22"}      # (the cluster stride: a sequence as b, as a, two profiles)
    assert mj.TARGETS == [31, 32, 33, 63, 64, 65, 127, 128, 129]
    for kind in ("ss", "ps", "sp", "pp22"):            # the four instances of the batched loop meet every edge, in every alphabet
        mine = [j for j in JOBS if j[0] == kind and j[3] == "plain"]
        assert set(mj.TARGETS) <= {j[1] for j in mine}, kind
        assert {j[2] for j in mine} == set(mj.ALPHABETS), kind
    assert {j[3] for j in JOBS} == set(mj.SCORINGS)
    assert [(int(m.get("KA_MERGE", 15)), m.get("KA_MAX_CLUSTER")) for m in mj.MODES] == [(k, c) for k in (15, 0, 1, 3, 7) for c in (None, "1")]
    for j in JOBS:
        codes, tasks, dist = mj.job(*j)
        assert 2 < len(codes) <= 6 and len(tasks) == len(codes) - 1 and len(dist) == len(codes), j
        assert [int(c) for c in tasks[:, 2]] == list(range(len(codes), 2 * len(codes) - 1)), j
        top = max(int(c.max()) for c in codes)
        assert top <= {"protein": 19, "bzx": 22, "dna": 3}[j[2]], j
        if j[2] == "bzx":
            assert all(int(c.max()) >= 20 for c in codes), j
        _, scal = mj.scoring(j)
        assert (scal[3] > 0 and scal[4] > 0) == (j[3] == "scaled") and float(scal[5]) == {"w1": 1.0, "w025": 0.25}.get(j[3], 0.0), j


def test_refine_codes_are_all_that_convert_raw_path_emits(oracle):
    """every raw path of operands of up to 5 x 5 letters that has a match (a raw path: per letter of a its column in b, ascending,
    or -1): the values ko_convert_raw_path emits are exactly mj.REFINE_CODES"""
    L = oracle.lib()
    seen, abutting = set(), set()
    for la, lb in itertools.product(range(1, 6), repeat=2):
        for k in range(1, min(la, lb) + 1):
            for ia in itertools.combinations(range(1, la + 1), k):
                for ib in itertools.combinations(range(1, lb + 1), k):
                    raw = np.full(la + 2, -1, np.int32)
                    raw[list(ia)] = ib
                    out = np.zeros(la + lb + 3, np.int32)
                    L.ko_convert_raw_path(raw.ctypes.data_as(C.c_void_p), la, lb, out.ctypes.data_as(C.c_void_p))
                    ops = out[1:out[0] + 1]
                    # a run in a directly behind a run in b: no path of the DP has one (both passes enter a gap state from
                    # the match state or from itself only); kept apart
                    abut = bool((((ops[:-1] & 3) == 2) & ((ops[1:] & 3) == 1)).any())
                    (abutting if abut else seen).update(ops.tolist())
    assert seen == set(mj.REFINE_CODES) and len(mj.REFINE_CODES) == 17
    assert abutting - seen == {1}                      # (its first column, flagless, is the one value a DP path cannot show)
    # ... and it names what the issue names: open, extension, close, a one-column run, a leading one-column terminal run, the
    # first column of a trailing run -- for a gap in a (1) and in b (2)
    assert all(op | f in mj.REFINE_CODES for op in (1, 2) for f in (4, 8, 16, 4 | 16, 16 | 32, 4 | 32))


@pytest.mark.parametrize("j", JOBS, ids=mj.job_id)
def test_target_node_has_the_listed_length(oracle, j):
    """plen + 2 of the target node, exactly -- in the first pass, in default mode and after refinement alike"""
    t = mj.target_task(j)
    for n_anchors, refine in ((0, 0), (3, 0), (0, 1), (0, 3)):
        recs, _, _ = mj.want(j, n_anchors, refine)
        assert recs[t].plen + 2 == j[1], (j, n_anchors, refine)
        assert (recs[t].nsip_a, recs[t].nsip_b) == tuple(len(m) for m in mj.TREES[j[0]][3:5]), j
    recs, _, _ = mj.want(j)
    if j[1] == mj.BIG:
        assert min(recs[t].len_a, recs[t].len_b) >= 320, j


@pytest.mark.parametrize("j", PLANNED, ids=mj.job_id)
def test_target_path_is_the_planned_one(oracle, j):
    """a terminal gap run at both ends, of |X| and |Y| columns, one in each operand; inside, exactly one gap run in each
    operand, of the planned lengths"""
    x, y, run_a, run_b, x_first = mj.plan_of(j)
    path = _target_path(j)
    assert set(mj.FIRST_CODES) == set(np.asarray(path[1:path[0] + 1]).tolist()), j
    runs = mj.runs_of(path)
    # X is a's: where a has letters and b none, the gap is in b (op 2)
    first, last = ((2, 1, x, True), (1, path[0] - y + 1, y, True)) if x_first else ((1, 1, y, True), (2, path[0] - x + 1, x, True))
    assert runs[0] == first and runs[-1] == last, (j, runs)
    inner = sorted((op, n) for op, _, n, term in runs if not term)
    assert inner == [(1, run_a), (2, run_b)], (j, runs)


@pytest.mark.parametrize("j", PROFILE_JOBS, ids=mj.job_id)
def test_profile_operands_arrive_with_gap_columns(oracle, j):
    """the gap counts are non-zero in every profile operand of the target and in the target's own output: field 24 (columns of
    a run inside) and 25 (of a terminal run) in the first pass, whose codes carry no open / close flag; after refinement 23
    (a run's first and last column; 24 is left to the columns between them, and the members' own runs are one and two long)"""
    for refine in (0, 1):
        nodes, _ = mj.expected(j, 0, refine)
        recs, _, _ = mj.want(j, 0, refine)
        r = recs[mj.target_task(j)]
        for x, n in ((r.a, r.nsip_a), (r.b, r.nsip_b)):
            if n > 1:
                assert nodes[x][1:-1, 23 if refine else 24].any(), (j, refine, x)
        assert nodes[r.c][1:-1, 23 if refine else 24].any() and nodes[r.c][1:-1, 25].any(), (j, refine)
        if j[2] == "bzx":
            assert nodes[r.c][1:-1, 20:23].any(), j


def test_every_code_and_run_length_is_met(oracle):
    # first pass: every code in the target path of some job of each kind (in fact of every planned job, above) ...
    for kind in mj.KINDS:
        seen = set()
        for j in JOBS:
            if j[0] == kind:
                p = _target_path(j)
                seen |= set(np.asarray(p[1:p[0] + 1]).tolist())
        assert seen == set(mj.FIRST_CODES), kind
    # ... and in the non-root tasks of every kind of RECORD, either way round
    recs_kinds = {}
    for j in JOBS:
        recs, paths, _ = mj.want(j)
        for t in range(len(recs) - 1):
            p = _path(recs, paths, t)
            recs_kinds.setdefault((recs[t].kind, recs[t].nsip_a > 1, recs[t].nsip_b > 1), set()).update(np.asarray(p[1:p[0] + 1]).tolist())
    assert set(recs_kinds) == {(mj.SS, False, False), (mj.SP, True, False), (mj.SP, False, True), (mj.PP, True, True)}
    assert all(v == set(mj.FIRST_CODES) for v in recs_kinds.values()), recs_kinds
    # gap runs of 1, 2 and 5 or more columns inside either operand, terminal ones of 1 and 3 at either end of either operand
    inner, term = set(), set()
    for j in PLANNED:
        p = _target_path(j)
        for op, c, n, t in mj.runs_of(p):
            (term if t else inner).add((op, c == 1, min(n, 5)) if t else (op, min(n, 5)))
    assert {(op, n) for op in (1, 2) for n in (1, 2, 5)} <= inner
    assert {(op, front, n) for op in (1, 2) for front in (True, False) for n in (1, 3)} <= term
    # refinement: every value convert_raw_path can emit, in a non-root path of some job
    seen = set()
    for j in JOBS:
        for p in _nonroot_paths(j, refine=1):
            seen |= set(np.asarray(p[1:p[0] + 1]).tolist())
    assert seen == set(mj.REFINE_CODES), sorted(set(mj.REFINE_CODES) - seen)
    # (mode 3, inline refinement, codes its paths as the first pass does)
    assert all(set(np.asarray(p[1:p[0] + 1]).tolist()) <= set(mj.FIRST_CODES) for j in JOBS for p in _nonroot_paths(j, refine=3))


def test_every_listed_length_is_met_exactly(oracle):
    got = set()
    for j in JOBS:
        recs, _, _ = mj.want(j)
        got |= {recs[t].plen + 2 for t in range(len(recs) - 1)}
    assert {3, 4} | set(mj.TARGETS) <= got
    # (a leaf's records: one float4 per thread in a plain loop, no batches; the shortest there are, and some past a stride)
    lens = {len(c) + 2 for j in JOBS for c in mj.job(*j)[0]}
    assert {3, 4} <= lens and max(lens) > 320


def test_the_scaled_jobs_carry_scaled_penalties_into_their_leaf_records(oracle):
    for j in JOBS:
        recs, _, _ = mj.want(j)
        _, scal = mj.scoring(j)
        _, leaves = mj.expected(j)
        for r in recs:
            assert (r.gap_scale < 1.0 and r.subm_off > 0.0) == (j[3] == "scaled"), (j, r.gap_scale, r.subm_off)
            for x, n in ((r.a, r.nsip_a), (r.b, r.nsip_b)):
                if n == 1:
                    assert leaves[x][0, 55] == -np.float32(np.float32(scal[0]) * np.float32(r.gap_scale)), (j, x)
        assert sorted(leaves) == list(range(len(mj.job(*j)[0]))), j


@pytest.mark.parametrize("j", JOBS, ids=mj.job_id)
def test_recipe_hash_is_the_oracles(oracle, j):
    """every non-root node: first pass, default mode (three anchors), refinement modes 1 and 3"""
    for n_anchors, refine in ((0, 0), (3, 0), (0, 1), (0, 3)):
        recs, _, _ = mj.want(j, n_anchors, refine)
        nodes, _ = mj.expected(j, n_anchors, refine)
        assert sorted(nodes) == [recs[t].c for t in range(len(recs) - 1)]
        for t in range(len(recs) - 1):
            assert nodes[recs[t].c].shape == (recs[t].plen + 2, 64)
            assert _hash(oracle, nodes[recs[t].c]) == recs[t].prof_hash, (j, n_anchors, refine, t)


class _Rec:
    def __init__(self, g, t):
        self.gap_scale, self.subm_off = g.rec("gap_scale")[t], g.rec("subm_off")[t]
        self.path_off, self.plen = int(g.rec("path_off")[t]), int(g.rec("plen")[t])


@pytest.mark.parametrize("name", ["tree_prot32x200", "tree_prot24_scaled"])
def test_recipe_equals_the_reference_golden(oracle, name):
    """the real reference's records and paths in, its profile hashes of every task and its dumped profile, bit for bit, out"""
    g = Golden(name)
    nt = len(g.tasks)
    nodes, _ = mj.recipe(g.codes, g.tasks, g.subm, g.scal, [_Rec(g, t) for t in range(nt)], g.paths)
    for t in range(nt - 1):
        assert _hash(oracle, nodes[int(g.tasks[t][2])]) == int(g.rec("prof_hash")[t]), (name, t)
    d = nodes[int(g.tasks[int(g.dump_task)][2])].reshape(-1)
    assert len(d) == len(g.dump) and np.array_equal(d.view(np.uint32), g.dump.view(np.uint32))
