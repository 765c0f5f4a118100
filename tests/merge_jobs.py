"""Seeded jobs for the profile merge (ka_update_profile, ka_profile.h) and the leaf records (ka_make_leaf_profile): shared by
tests/test_gpu_merge.py, which runs them on the device and compares every merged record field by field, and
tests/test_merge_inputs.py, which checks on the host that every job is what it is listed for.  Host only: nothing here imports
the device library.

A job is a tiny tree (3 - 6 sequences) cut from one random core with planned edits, so that the coded path of its TARGET task --
the last task below the root, the one whose kind the job is named after -- is forced:
    operand a carries an overhang X at one end and lacks a run of the core; operand b carries an overhang Y at the other end
    and lacks another run.  The target's path then has a terminal gap run at both ends (codes 33 / 34) and one gap run inside
    each operand (codes 1 / 2), of the planned lengths, and plen = |X| + |core| + |Y|.
Every member of a profile operand shares its operand's edits; the members after the first lack one or two residues more, each
at its own place: the operand arrives at the target with gap columns of its own (count fields 23 - 25 non-zero on input).

The merge walks (column, float4) items, 16 to a column; one stride of a workgroup is blockDim.x / 16 columns -- 32 for the 8-wave
kernels, 16 for the 4-wave ones -- and a batched trip is KA_MERGE_BATCH = 4 strides, 128 or 64 columns.  TARGETS are the
plen + 2 either side of a stride and of a trip."""
import functools
import os

import numpy as np

import oracle_executor as ox
from util import GOLDEN

SS, SP, PP = 0, 1, 2                                  # a task record's `kind`

# kind -> (sequences, tasks, target task, members of the target's a, of its b); the last sequence is the root's other operand
TREES = {
    "ss":   (3, [(0, 1, 3), (3, 2, 4)], 0, [0], [1]),                                               # nsip 1 / 1
    "ps":   (4, [(0, 1, 4), (4, 2, 5), (5, 3, 6)], 1, [0, 1], [2]),                                 # 2 / 1: the profile is a
    "sp":   (5, [(0, 1, 5), (2, 5, 6), (3, 6, 7), (7, 4, 8)], 2, [3], [0, 1, 2]),                   # 1 / 3: the sequence is a (below it too, 1 / 2)
    "pp22": (5, [(0, 1, 5), (2, 3, 6), (5, 6, 7), (7, 4, 8)], 2, [0, 1], [2, 3]),                   # 2 / 2
    "pp32": (6, [(0, 1, 6), (6, 2, 7), (3, 4, 8), (7, 8, 9), (9, 5, 10)], 3, [0, 1, 2], [3, 4]),    # 3 / 2
}
KINDS = list(TREES)
ALPHABETS = ["protein", "bzx", "dna"]                 # codes 0-19; with B / Z / X (20-22: the count group k4 = 20 shares its float4 with field 23); 0-3
TARGETS = [31, 32, 33, 63, 64, 65, 127, 128, 129]     # plen + 2 of the target node
BIG = 342                                             # the root's child has >= 320 rows: its task, and so its merge, runs on two workgroups
SCORINGS = ["plain", "scaled", "w1", "w025"]          # scaled: dist_scale and vsm_amax > 0; w*: sequence weights scal[5] = 1.0 / 0.25

# (|X|, |Y|, gap run inside a, inside b, X at the front?) by the job's place in the table
PLANS = [(1, 3, 1, 5, True), (3, 1, 2, 1, False), (3, 3, 5, 2, True), (1, 1, 1, 2, False), (3, 1, 6, 1, True), (1, 3, 2, 7, False)]

# KA_MERGE: bit 0 the batched loop for two profiles, bit 1 with a sequence made from its residue, bit 2 on a cluster, bit 3 in
# the 128-register units; unset = 15.  0 is the one-item loop everywhere.
MODES = [dict(m, **c) for m in ({}, {"KA_MERGE": "0"}, {"KA_MERGE": "1"}, {"KA_MERGE": "3"}, {"KA_MERGE": "7"}) for c in ({}, {"KA_MAX_CLUSTER": "1"})]
MODE_KEYS = ["KA_MERGE", "KA_MAX_CLUSTER"]

# Codes of a first-pass path (ko_code_path: add_gap_info_to_path_n as executed sets the terminal flag only)
FIRST_CODES = [0, 1, 2, 33, 34]
# Codes of a refined path, derived from ko_convert_raw_path.  op = 1 (gap in a) or 2 (gap in b).  The flag loop starts at the
# SECOND column and stops at the terminator, then the terminal runs get 32:
#   inside:    op|4 opens a run of two or more, op|8 extends one of three or more, op|16 closes one of two or more (the
#              loop turns the 8 of the run's last column into 16), op|4|16 is a run of one column;
#   leading:   the first column is never opened: op|32 alone, then op|8|32, closed by op|16|32 -- which is also the whole of a
#              leading run of one column;
#   trailing:  opened by op|4|32, extended by op|8|32, never closed (the loop ends on the terminator);
#   a run in a directly behind a run in b would leave its first column a bare 1, the one further value the function can emit;
#   no path of the DP has such a pair (a gap state is entered from the match state or from itself only), so it is not listed.
# tests/test_merge_inputs.py holds this list against every raw path of two short operands.
REFINE_CODES = [0] + [op | f for op in (1, 2) for f in (4, 8, 16, 4 | 16, 32, 8 | 32, 16 | 32, 4 | 32)]

# The seed of a job is its base seed plus the bump listed here, for the jobs whose base seed misses a condition of
# tests/test_merge_inputs.py.  What each one missed is noted next to it.
SEED_BUMP = {
    # the path left the plan: a planned run inside was not taken (the letters next to it matched by chance and the run moved,
    # merged with the terminal run or split in two); with it the target's length was off for the ones marked *
    ("ss", 65, "dna", "plain"): 1, ("ps", 64, "dna", "plain"): 1,       # *: 66 for 64
    ("sp", 31, "dna", "plain"): 3,                                      # *: 29 for 31
    ("sp", 33, "bzx", "plain"): 1,                                      # *: 29 for 33
    ("sp", 63, "dna", "plain"): 2,
    ("pp32", 33, "protein", "plain"): 2,                                # *: 32 for 33
    ("ps", 32, "dna", "w1"): 1,                                         # *: 28 for 32
}


def jobs():
    """(kind, target, alphabet, scoring): every target for the four instances of the batched loop (which operand is a sequence),
    the alphabet rotating; 3 / 2 at one target per stride and trip; two sequences of length 1 (plen + 2 = 3) and of 1 and 2 (4);
    the two-workgroup jobs, one per instance of the batched loop that a cluster can run; scaled penalties; sequence weights"""
    out = []
    for k, kind in enumerate(["ss", "ps", "sp", "pp22"]):
        out += [(kind, t, ALPHABETS[(k + i) % 3], "plain") for i, t in enumerate(TARGETS)]
    out += [("pp32", 33, "protein", "plain"), ("pp32", 64, "bzx", "plain"), ("pp32", 127, "dna", "plain")]
    out += [("ss", 3, "protein", "plain"), ("ss", 3, "dna", "plain"), ("ss", 4, "bzx", "plain"), ("ss", 4, "dna", "plain")]
    # (no seq-seq one: a level of seq-seq tasks goes to the 128-register units, one workgroup per task, whatever its rows)
    out += [("pp22", BIG, "protein", "plain"), ("ps", BIG, "dna", "plain"), ("sp", BIG, "bzx", "plain")]
    out += [("sp", 65, "protein", "scaled"), ("ps", 33, "bzx", "scaled")]
    out += [("pp32", 65, "protein", "w1"), ("ps", 32, "dna", "w1"), ("pp22", 129, "bzx", "w025"), ("ss", 63, "protein", "w025")]
    return out


def job_id(job):
    return "%s-%d-%s-%s" % job


def seed_of(job):
    kind, target, alphabet, scoring = job
    base = 100000 * (1 + KINDS.index(kind)) + 37 * target + 30000 * ALPHABETS.index(alphabet) + 7000 * SCORINGS.index(scoring)
    return base + SEED_BUMP.get(job, 0)


def plan_of(job):
    kind, target, alphabet, scoring = job
    x, y, run_a, run_b, x_first = PLANS[(KINDS.index(kind) + TARGETS.index(target) if target in TARGETS else 2) % len(PLANS)]
    if alphabet == "dna" and target < 60:
        # four letters, terminal gaps for nothing (tgpe = 0) and a core of some 25 letters: a run of five columns inside is never
        # the best path there, whatever the seed -- the short dna jobs plan runs of one and two
        run_a, run_b = min(run_a, 2), min(run_b, 2)
    return x, y, run_a, run_b, x_first


def scoring(job):
    """(subm, scal): the plain tables of param_tables.npz; `scaled` and the sequence weights change scal only"""
    z = np.load(os.path.join(GOLDEN, "param_tables.npz"))
    subm, scal = (z["subm_1_0"], z["scal_1_0"].copy()) if job[2] == "dna" else (z["subm_0_3"], z["scal_0_3"].copy())
    scal[3], scal[4], scal[5] = {"plain": (0.0, 0.0, 0.0), "scaled": (0.5, 2.0, 0.0), "w1": (0.0, 0.0, 1.0), "w025": (0.0, 0.0, 0.25)}[job[3]]
    return subm, scal


def _cut(core, lacks):
    keep = np.ones(len(core), bool)
    for p, d in lacks:
        assert keep[p:p + d].all() and p + d < len(core)
        keep[p:p + d] = False
    return core[keep]


@functools.lru_cache(maxsize=None)
def job(kind, target, alphabet, scoring_name):
    """(codes, tasks, seq_distances) -- the root is the last task, the target the one before it"""
    rng = np.random.RandomState(seed_of((kind, target, alphabet, scoring_name)))
    alpha = 4 if alphabet == "dna" else 20
    nseq, tasks, _, mem_a, mem_b = TREES[kind]
    if target <= 4:
        # two sequences of length 1 (one column), of 1 and 2 (a terminal gap next to the only match); no room for planned edits
        a = rng.randint(0, alpha, 1).astype(np.uint8)
        codes = [a, a.copy() if target == 3 else np.concatenate([a, rng.randint(0, alpha, 1).astype(np.uint8)]), np.concatenate([a, a])]
    else:
        x, y, run_a, run_b, x_first = plan_of((kind, target, alphabet, scoring_name))
        n = target - 2 - x - y
        core = rng.randint(0, alpha, n).astype(np.uint8)
        X, Y = rng.randint(0, alpha, x).astype(np.uint8), rng.randint(0, alpha, y).astype(np.uint8)
        codes = [None] * nseq
        for side, members in enumerate((mem_a, mem_b)):
            shared = (n // 5, run_a) if side == 0 else ((7 * n) // 10, run_b)
            for m, s in enumerate(members):
                lacks = [shared]
                if m:                                             # one or two residues of its own: gap columns inside the operand
                    lacks.append(((n // 2 if side == 0 else (7 * n) // 20) + 3 * (m - 1), 1 + (m + side) % 2))
                body = _cut(core, lacks)
                sub = rng.rand(len(body)) < 0.08
                body[sub] = rng.randint(0, alpha, int(sub.sum()))
                front = (side == 0) == x_first
                codes[s] = np.concatenate([X if side == 0 else Y, body]) if front else np.concatenate([body, X if side == 0 else Y])
        last = core.copy()
        sub = rng.rand(n) < 0.08
        last[sub] = rng.randint(0, alpha, int(sub.sum()))
        codes[nseq - 1] = last
    if alphabet == "bzx":
        for c in codes:
            idx = rng.randint(0, len(c), max(len(c) // 12, 1))
            c[idx] = rng.randint(20, 23, len(idx)).astype(np.uint8)
    codes = [np.ascontiguousarray(c, np.uint8) for c in codes]
    for c in codes:
        c.setflags(write=False)
    return codes, np.array(tasks, np.int32), np.linspace(0.2, 1.1, nseq).astype(np.float32)


def target_task(j):
    return TREES[j[0]][2]


@functools.lru_cache(maxsize=None)
def want(j, n_anchors=0, refine=0):
    """the oracle's answer: (records, coded paths, gap arrays) of the first pass, of the first pass in default mode (n_anchors),
    or of refinement mode `refine`"""
    from oracle import oracledrv
    codes, tasks, dist = job(*j)
    subm, scal = scoring(j)
    if refine:
        return oracledrv.msa_tree_refine(list(codes), tasks, subm, scal, dist, refine, None, n_anchors)
    if n_anchors:
        return oracledrv.msa_tree_cons(list(codes), tasks, subm, scal, dist, n_anchors, 2.0)[:3]
    return oracledrv.msa_tree(list(codes), tasks, subm, scal, dist)[:3]


def recipe(codes, tasks, subm, scal, recs, paths):
    """The expected records of a run whose task records and coded paths are given, by ko_msa_tree's own sequence of the oracle's
    primitives (oracle_executor's: make_profile_n for the task's penalties, set_gap_penalties_n on a copy, update_n along the
    coded path): (nodes, leaves).  nodes[c] = the merged profile of every non-root node, (plen + 2) x 64 floats AS CREATED --
    before the task that consumes it sets fields 27 - 29; leaves[i] = the (len + 2) x 64 records of sequence i, made with the
    penalties and the score offset of the task that consumes it."""
    subm = np.ascontiguousarray(subm, np.float32).reshape(-1)
    n = len(codes)
    nsip, plen, prof = {i: 1 for i in range(n)}, {i: len(c) for i, c in enumerate(codes)}, {}
    nodes, leaves = {}, {}
    for t, (a, b, c) in enumerate(np.asarray(tasks).tolist()):
        r = recs[t]
        pen = ox.task_penalties(scal, r.gap_scale, r.subm_off)
        pa, pb = ox.task_operands(codes, subm, pen, a, b, nsip, plen, prof)
        for x, p in ((a, pa), (b, pb)):
            if nsip[x] == 1:
                leaves[x] = p.reshape(-1, 64)
        coded = np.asarray(paths[r.path_off:r.path_off + r.plen + 2], np.int32)
        nsip[c], plen[c] = nsip[a] + nsip[b], int(coded[0])
        if t != len(tasks) - 1:
            prof[c] = ox.merged_profile(pa, pb, coded, nsip[a], nsip[b], subm, scal)
            nodes[c] = prof[c].reshape(-1, 64)
    return nodes, leaves


@functools.lru_cache(maxsize=None)
def expected(j, n_anchors=0, refine=0):
    codes, tasks, _ = job(*j)
    recs, paths, _ = want(j, n_anchors, refine)
    subm, scal = scoring(j)
    return recipe(list(codes), tasks, subm, scal, recs, paths)


def runs_of(path):
    """[(op, first column, length, terminal?)] of the gap runs of a coded path"""
    ops = np.asarray(path[1:int(path[0]) + 1])
    out, c = [], 0
    while c < len(ops):
        op = int(ops[c]) & 3
        e = c
        while e < len(ops) and (int(ops[e]) & 3) == op:
            e += 1
        if op:
            out.append((op, c + 1, e - c, bool(ops[c] & 32)))
        c = e
    return out
