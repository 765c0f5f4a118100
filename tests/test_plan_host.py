"""CPU: the launch planner (kalign_amd/csrc/ka_plan.cpp) without a GPU.  ka_debug_plan prepares and plans a job as ka_tree_upload
does; every case and switch set of tests/golden/plan_*.npz (make_golden_plan.py: recorded from the single-function planner of
round 6) must come out as stored -- array for array, or scalar for scalar and digest for digest -- and every plan with a chained
launch must be one the device can run: the whole launch resident, every join count the number of arrivals."""
import os
import sys

import numpy as np
import pytest

from util import GOLDEN

sys.path.insert(0, GOLDEN)
import make_golden_plan as mp  # noqa: E402

PLANS = [(name, k) for name in sorted(mp.CASES) for k in range(len(mp.CASES[name][5]))]

_jobs, _files = {}, {}


def job_of(name):
    if name not in _jobs:
        _jobs[name] = mp.case_inputs(name)
    return _jobs[name]


def file_of(name):
    if name not in _files:
        _files[name] = np.load(os.path.join(GOLDEN, "plan_%s.npz" % name))
    return _files[name]


def test_names_and_abi_version():
    from kalign_amd import api
    L = api.load_library()
    assert L.ka_abi_version() >= 27
    for name in ("ka_debug_plan", "ka_debug_ctx_plan"):
        assert name in api.EXPORTS and hasattr(L, name), name


@pytest.mark.parametrize("name", sorted(mp.CASES))
def test_inputs_are_the_recorded_ones(name):
    z = file_of(name)
    assert mp.input_digests(job_of(name)).tolist() == z["inputs_sha256"].tolist()
    sets = mp.CASES[name][5]
    assert z["switches"].tolist() == [" ".join("%s=%s" % kv for kv in sorted(s.items())) for s in sets]


def levels_of(job):
    n = len(job["lens"])
    level = np.zeros(2 * n - 1, np.int64)
    for a, b, c in job["tasks"]:
        level[c] = 1 + max(level[a], level[b])
    return level[job["tasks"][:, 2]] - 1


def check_invariants(job, plan):
    """what the device relies on in a plan with a chained launch"""
    tasks, n_tasks, n = job["tasks"], len(job["tasks"]), len(job["lens"])
    active = np.ones(n_tasks, bool)
    if job["task_ids"] is not None:
        active[:] = False
        active[job["task_ids"]] = True
    level = levels_of(job)
    in_chain = active & (level >= plan["chain_level"])
    task_of = {int(c): t for t, (_, _, c) in enumerate(tasks)}
    # join counts: the children that run inside the launch (plus the one that never comes, under the starve hook)
    need = np.zeros(n_tasks, np.int64)
    for t in np.flatnonzero(in_chain):
        need[t] = sum(1 for ch in tasks[t, :2] if ch >= n and in_chain[task_of[int(ch)]])
    if job["hooks"] & mp.STARVE_ROOT_JOIN:
        need[n_tasks - 1] += 1
    assert np.array_equal(plan["chain_need"], need)
    # The chain's table holds the launch's ENTRIES -- its tasks with no child inside it -- each with members 0 .. g-1 exactly
    # once; every other task of the launch is reached from them through the join points (a parent inside the launch).
    t_blk, member, g = mp.chain_table(plan)
    entries = {int(t) for t in np.flatnonzero(in_chain) if plan["chain_need"][t] == 0}
    assert set(t_blk.tolist()) == entries
    for t in entries:
        sel = t_blk == t
        gt = int(g[sel][0])
        assert (g[sel] == gt).all() and sorted(member[sel].tolist()) == list(range(gt)), t
    reached = np.zeros(n_tasks, bool)
    for t in entries:
        while t >= 0 and not reached[t]:
            reached[t] = True
            t = int(plan["parent"][t])
            assert t < 0 or in_chain[t]
    assert np.array_equal(reached, in_chain)
    assert len(t_blk) <= job["n_cus"]                                         # resident at once
    # no flag bits in the block table: a workgroup's second word is member | cluster size << 8
    assert (plan["blocks"][plan["blocks"][:, 0] >= 0, 1] < (1 << 16)).all()
    # the queued launch: exactly the plan's tasks of levels queue_first .. chain_level - 1, each once, producers before consumers
    q = plan["blocks"][plan["queue_off"]:plan["queue_off"] + plan["queue_n"], 0]
    if plan["queue_first"] >= 0:
        queued = np.flatnonzero(active & (level >= plan["queue_first"]) & (level < plan["chain_level"]))
        assert sorted(q.tolist()) == queued.tolist()
    else:
        assert len(q) == 0
    pos = {int(t): i for i, t in enumerate(q)}
    for i, t in enumerate(q):
        for p in (int(plan["qa"][t]), int(plan["qb"][t])):
            assert p < 0 or pos[p] < i, (int(t), p)


@pytest.mark.parametrize("name,k", PLANS)
def test_plan_is_the_recorded_one(name, k):
    from kalign_amd import api
    job, z = job_of(name), file_of(name)
    plan = mp.plan_of(job, mp.CASES[name][5][k])
    assert dict(zip(api.PLAN_SCALARS, mp.scalars(plan).tolist())) == dict(zip(api.PLAN_SCALARS, z["s%d_scalars" % k].tolist()))
    assert mp.summary(plan).tolist() == z["s%d_summary" % k].tolist()
    for i, a in enumerate(mp.ARRAYS):
        if mp.CASES[name][4]:
            assert np.array_equal(plan[a], z["s%d_%s" % (k, a)]), a
        else:
            assert mp.sha(plan[a]) == str(z["s%d_sha256" % k][i]), a
    if plan["chain_level"] >= 0:
        check_invariants(job, plan)


def test_fixtures_reach_every_branch():
    mp.check_coverage({name: file_of(name) for name in mp.CASES})


def test_switches_are_read_on_every_call_and_do_not_leak(monkeypatch):
    """ka_debug_plan reads the environment itself: a switch set between two calls changes the second plan, and unsetting it
    gives the first again"""
    from kalign_amd import api
    job = job_of("b")
    for k in mp.PLAN_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    base = api.debug_plan(job["lens"], job["tasks"], job["n_cus"])
    monkeypatch.setenv("KA_NO_CHAIN", "1")
    assert api.debug_plan(job["lens"], job["tasks"], job["n_cus"])["chain_level"] == -1 and base["chain_level"] >= 0
    monkeypatch.delenv("KA_NO_CHAIN")
    again = api.debug_plan(job["lens"], job["tasks"], job["n_cus"])
    assert all(np.array_equal(base[a], again[a]) for a in mp.ARRAYS)


def test_a_task_list_out_of_order_is_refused():
    """the seam refuses what ka_tree_upload refuses, with its message"""
    from kalign_amd import api
    job = job_of("a")
    tasks = job["tasks"].copy()
    tasks[[0, len(tasks) - 1]] = tasks[[len(tasks) - 1, 0]]          # the root first: its children are not made yet
    with pytest.raises(api.KalignAmdError, match=r"task list is not in TASK_ORDER_TREE order \(children before parents\)"):
        api.debug_plan(job["lens"], tasks, job["n_cus"])
    tasks = job["tasks"].copy()
    tasks[1, 0] = tasks[0, 0]                                         # a node consumed by two tasks
    with pytest.raises(api.KalignAmdError, match=r"task list is not in TASK_ORDER_TREE order \(a node is consumed twice\)"):
        api.debug_plan(job["lens"], tasks, job["n_cus"])
