"""Writes tests/golden/plan_*.npz: the launch plans of the planner (kalign_amd/csrc/ka_plan.cpp: plan_launches) for seeded jobs, one
file per case, one plan per set of KA_* switches -- through ka_debug_plan, which needs no GPU.

    python tests/golden/make_golden_plan.py [--dump DIR] [CASE ...]       (needs the built library)

The inputs (guide tree, lengths, task subset) are regenerated from seeds by case_inputs(); a file holds their sha256 only.  Per
switch set k a file holds `s<k>_scalars` (api.PLAN_SCALARS), `s<k>_summary` (SUMMARY, what the coverage assertions read) and either
every array of the flattened plan (`s<k>_<name>`, the small cases) or `s<k>_sha256`, one digest per array in ARRAYS order.
--dump DIR writes every array of every plan to DIR/<case>_s<k>.npz, to see WHAT differs when a digest does.

The fixtures in the repository were recorded when ka_debug_plan was first put around the planner, with plan_launches still the
single function it had been since round 6: they pin that function's plans, and every later form of the planner must reproduce them.
When the planner's round-6 experiments left (spines, kept CUs, one queue order, b / a as a switch) the files were CONVERTED, not
recorded again: their five switch sets dropped and the others renumbered, the "CUs kept" scalar, the spine count of the summary and
the spine array (all zeros in every plan that stayed) taken out, every other stored value as it was.
"""
import contextlib
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

ARRAYS = ("parent", "chain_need", "is_root", "wait_mult", "qa", "qb", "blocks", "blocks_off", "level_lean")
SUMMARY = ("lean_mask", "entry_g_min", "entry_g_max")
STARVE_ROOT_JOIN = 2                  # KA_DEBUG_STARVE_ROOT_JOIN
ALL_SWITCHES = ({}, {"KA_QORDER": "0"}, {"KA_NO_CRIT": "1"}, {"KA_CRIT_GREEDY": "0"}, {"KA_CRIT_TOP": "8"}, {"KA_CHAIN_G1": "1"},
                {"KA_NO_CHAIN": "1"}, {"KA_NO_QUEUE": "1"}, {"KA_NO_HALF": "1"}, {"KA_NO_LEAN": "1"}, {"KA_OVERLAP": "0"},
                {"KA_MAX_CLUSTER": "4"}, {"KA_CHAIN_TASKS": "64"})
# every switch the planner reads: none of them may leak in from the caller's environment
PLAN_SWITCHES = sorted({k for s in ALL_SWITCHES for k in s} | {"KA_PLAN_VERBOSE"})
CASES = {
    # name: (sequences, (shortest, longest) length, seed, n_cus, stores every array, switch sets, what else)
    "a": (40, (80, 320), 11, 256, True, ({},), {}),
    "b": (700, (150, 450), 12, 64, True, ALL_SWITCHES, {}),
    "c": (2560, (270, 330), 5, 256, False, ALL_SWITCHES, {}),
    "d": (4096, (340, 460), 14, 256, False, ({},), {}),
    "e": (1024, (1800, 2200), 15, 256, False, ({},), {}),
    "f": (2048, (200, 400), 16, 256, False, ({},), {"cons_K": 5}),
    "g": (700, (150, 450), 12, 64, False, ({},), {"copies": 16}),
    "h": (300, (200, 600), 18, 256, False, ({},), {"caterpillar": True}),
    "i": (2560, (270, 330), 5, 256, False, ({},), {"rank_of": 2}),
    "j": (700, (150, 450), 12, 64, True, ({},), {"shared": True}),
    "k": (700, (150, 450), 12, 64, True, ({},), {"hooks": STARVE_ROOT_JOIN}),
    # (b and c fill their CUs with entries: no spare workgroups.  A tree that leaves some, so that the KA_CRIT_* sets differ)
    "l": (3072, (340, 460), 19, 256, False, ALL_SWITCHES, {}),
}


def caterpillar(n, seed):
    """the narrowest tree: a spine that takes up one sequence after the other, in a seeded order"""
    order = np.random.RandomState(seed).permutation(n)
    tasks, cur = [], int(order[0])
    for t in range(n - 1):
        tasks.append((cur, int(order[t + 1]), n + t))
        cur = n + t
    return np.array(tasks, np.int32)


def case_inputs(name):
    """the job of a case, regenerated from its seeds: dict(lens, tasks, n_cus, shared, cons_K, hooks, task_ids)"""
    from kalign_amd import api, guide
    n, (lo, hi), seed, n_cus, _, _, more = CASES[name]
    lens = np.random.RandomState(seed).randint(lo, hi + 1, n).astype(np.int32)
    tasks = caterpillar(n, seed) if more.get("caterpillar") else guide.bisecting_tree(n, seed=seed)
    if more.get("copies"):
        _, tasks, _, _ = guide.forest([(range(n), tasks)] * more["copies"])
        lens = np.tile(lens, more["copies"])
    task_ids = None
    if more.get("rank_of"):                          # rank 0's subtrees of the tree cut for that many ranks
        run_rank, top = api.dist_plan_subtrees(lens, tasks, more["rank_of"])
        task_ids = np.array([t for t in range(len(tasks)) if run_rank[t] == 0 and t not in set(top)], np.int32)
    return dict(lens=lens, tasks=np.ascontiguousarray(tasks, np.int32), n_cus=n_cus, shared=bool(more.get("shared")),
                cons_K=more.get("cons_K", 0), hooks=more.get("hooks", 0), task_ids=task_ids)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.int32).tobytes()).hexdigest()


def input_digests(job):
    ids = job["task_ids"] if job["task_ids"] is not None else np.zeros(0, np.int32)
    return np.array([sha(job["lens"]), sha(job["tasks"]), sha(ids)])


@contextlib.contextmanager
def switched(switches):
    """the environment with exactly these planner switches set, put back afterwards"""
    saved = {k: os.environ.pop(k, None) for k in PLAN_SWITCHES}
    os.environ.update(switches)
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def plan_of(job, switches):
    from kalign_amd import api
    with switched(switches):
        return api.debug_plan(job["lens"], job["tasks"], job["n_cus"], job["shared"], job["cons_K"], job["hooks"], job["task_ids"])


def chain_table(plan):
    """the chained launch's block table: (task, member, cluster size) of its non-empty blocks"""
    b = plan["blocks"][plan["chain_blocks_off"]:plan["chain_blocks_off"] + plan["chain_blocks_n"]]
    b = b[b[:, 0] >= 0]
    return b[:, 0], b[:, 1] & 0xff, (b[:, 1] >> 8) & 0xff


def summary(plan):
    """SUMMARY: which launch kinds the levels have (bit k: kind k); fewest and most workgroups of a chain entry"""
    _, _, g = chain_table(plan)
    return np.array([int(sum(1 << k for k in set(plan["level_lean"].tolist()))),
                     int(g.min()) if len(g) else 0, int(g.max()) if len(g) else 0], np.int32)


def scalars(plan):
    from kalign_amd import api
    return np.array([plan[k] for k in api.PLAN_SCALARS], np.int32)


def check_coverage(files):
    """files: {case: npz-like}.  Between them the cases reach every branch of the planner."""
    from kalign_amd import api
    sc, sm = [], []
    for z in files.values():
        for k in range(len(z["switches"])):
            sc.append(dict(zip(api.PLAN_SCALARS, z["s%d_scalars" % k].tolist())))
            sm.append(dict(zip(SUMMARY, z["s%d_summary" % k].tolist())))
    assert any(s["queue_first"] >= 0 and s["queue_n"] > 0 for s in sc), "no queued launch"
    assert any(s["overlap_plan"] > 0 for s in sc), "no overlapping launches"
    assert any(s["max_cluster"] == 32 for s in sc), "no cluster limit of 32"
    assert any(s["n_trees"] > 1 for s in sc), "no forest"
    assert any(s["chain_level"] == -1 for s in sc), "no plan without a chained launch"
    mask = 0
    for m in sm:
        mask |= m["lean_mask"]
    assert mask == 7, "launch kinds seen: mask %d" % mask
    assert any(m["entry_g_max"] > m["entry_g_min"] for m in sm), "no chain entry with spare workgroups"
    assert any(m["entry_g_min"] > 1 and s["max_cluster"] > 1 for m, s in zip(sm, sc)), "no chain that starts on more than one workgroup per entry"


def main(argv):
    dump = None
    if "--dump" in argv:
        dump = argv[argv.index("--dump") + 1]
        argv = [a for a in argv if a not in ("--dump", dump)]
        os.makedirs(dump, exist_ok=True)
    files = {}
    for name in (argv or sorted(CASES)):
        job = case_inputs(name)
        full, sets = CASES[name][4], CASES[name][5]
        out = dict(inputs_sha256=input_digests(job), switches=np.array([" ".join("%s=%s" % kv for kv in sorted(s.items())) for s in sets]))
        for k, s in enumerate(sets):
            plan = plan_of(job, s)
            out["s%d_scalars" % k], out["s%d_summary" % k] = scalars(plan), summary(plan)
            if full:
                out.update({"s%d_%s" % (k, a): plan[a] for a in ARRAYS})
            else:
                out["s%d_sha256" % k] = np.array([sha(plan[a]) for a in ARRAYS])
            if dump:
                np.savez_compressed(os.path.join(dump, "%s_s%d.npz" % (name, k)), **{a: plan[a] for a in ARRAYS})
            print("plan_%s %-28s %s summary %s" % (name, out["switches"][k] or "(default)", out["s%d_scalars" % k].tolist(), out["s%d_summary" % k].tolist()))
        files[name] = out
    if not argv:
        check_coverage(files)
    for name, out in files.items():
        np.savez_compressed(os.path.join(HERE, "plan_%s.npz" % name), **out)
    print("wrote %d files%s" % (len(files), "; coverage assertions passed" if not argv else ""))


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
