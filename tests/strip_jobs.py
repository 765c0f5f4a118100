"""Seeded jobs for the strip passes (ka_strip, ka_wstrip / ka_whelper, ka_packed) at their row and column edges: shared
by tests/test_gpu_strip_edges.py, which runs them on the device, and tests/test_strip_edge_inputs.py, which checks on the host that
the oracle's root task of every job really has the rows and columns it is here for.  Host only: nothing here imports the device
library."""
import functools
import os

import numpy as np

from util import GOLDEN

SS, SP, PP = 0, 1, 2                                  # a task record's `kind`

# (rows, cols) of the root task: rows is the operand the DP's rows run over (S.La), cols the one its columns run over
SHAPES = [
    # empty and one-row passes over long columns (they matter with KA_SUBTREE=0)
    (1, 200), (2, 321),
    # 64-row strips: passes of 63/64, 64/64, 64/65, 65/65 rows; the first sizes past the wide-subtree level (65 .. 128 rows)
    (127, 127), (128, 128), (128, 129), (129, 192), (130, 193), (129, 257),
    # 128-row strips (and 64-row ones): passes of 127/128, 128/128, 128/129 (a second strip of one row), 129/129, 129/130;
    # columns either side of a 64-column hand-over batch, and beyond 320 = 256 ring slots + one batch
    (255, 255), (256, 256), (257, 257), (257, 319), (257, 320), (258, 321), (259, 384), (256, 385),
    # three strips per pass, last strips of 127, 128, 1 and 2 rows; two workgroups per task (La >= 320)
    (511, 512), (512, 512), (513, 576), (514, 641),
]
# seq-profile only: a sequence shorter than the profile, and one much longer (the rows are always the profile)
SP_EXTRA = [(257, 64), (257, 65), (513, 63), (64, 513)]

KINDS = ["ss", "pp", "sp", "sp_mirror"]               # sp_mirror: the sequence as operand a (swapped = 1)
ALPHABETS = ["protein", "bzx", "dna"]                 # codes 0-19; with B / Z / X (20-22) sprinkled in: NRES = 23; codes 0-3

MODES = [{}, {"KA_HW": "0"}, {"KA_HW": "0", "KA_HO": "0"}, {"KA_HW": "0", "KA_HO": "2"}, {"KA_Q1": "0"}, {"KA_Q1": "0", "KA_HW": "0"},
         {"KA_Q1": "3", "KA_HW": "0"}, {"KA_Q1": "1"}, {"KA_MAX_CLUSTER": "1"}, {"KA_MAX_CLUSTER": "1", "KA_HW": "0"},
         {"KA_SUBTREE": "0"}, {"KA_SUBTREE": "0", "KA_HW": "0", "KA_HO": "0"}, {"KA_NO_CHAIN": "1"}, {"KA_MW": "0"}]
# with anchor consistency (no LDS hand-over there)
CONS_MODES = [{}, {"KA_HW": "0"}, {"KA_Q1": "0"}, {"KA_MAX_CLUSTER": "1"}, {"KA_SUBTREE": "0"}]
MODE_KEYS = sorted({k for m in MODES for k in m})

# The seed of a job is its base seed plus the bump listed here.  Bumped are the jobs whose base seed misses what
# tests/test_strip_edge_inputs.py asserts.  All ten missed the same condition: their root path had no gap run inside each
# operand.  No job needed a bump for its profile lengths: every profile came out as long as its two sequences at the base seed.
# (kind "sp" stands for both orientations: they share their sequences.)
SEED_BUMP = {
    ("ss", 129, 192, "dna"): 1, ("ss", 129, 257, "dna"): 1, ("pp", 255, 255, "dna"): 1, ("sp", 128, 129, "dna"): 4,
    ("sp", 129, 192, "dna"): 1, ("sp", 130, 193, "dna"): 2, ("sp", 257, 64, "dna"): 1, ("sp", 257, 65, "dna"): 1,
    ("sp", 513, 63, "dna"): 1, ("sp", 64, 513, "dna"): 8,
}


def shapes(kind):
    return SHAPES + (SP_EXTRA if kind.startswith("sp") else [])


def cases():
    return [(k, r, c, a) for k in KINDS for (r, c) in shapes(k) for a in ALPHABETS]


def cons_cases():
    """default mode (anchor consistency): the profile tasks of the shapes with 128-row strips"""
    return [(k, r, c, a) for (k, r, c, a) in cases() if k != "ss" and r >= 255]


def case_id(case):
    return "%s-%dx%d-%s" % case


def seed_of(kind, rows, cols, alphabet):
    k = "sp" if kind == "sp_mirror" else kind
    base = 100000 * (1 + ["ss", "pp", "sp"].index(k)) + 31 * rows + 7 * cols + 50000 * ALPHABETS.index(alphabet)
    return base + SEED_BUMP.get((k, rows, cols, alphabet), 0)


def scoring(alphabet):
    z = np.load(os.path.join(GOLDEN, "param_tables.npz"))
    return (z["subm_1_0"], z["scal_1_0"].copy()) if alphabet == "dna" else (z["subm_0_3"], z["scal_0_3"].copy())


def _copy(rng, s, alpha):
    """substitutions only (about 10 %): s and its copy align to a profile of exactly len(s) columns"""
    t = s.copy()
    m = rng.rand(len(t)) < 0.1
    t[m] = rng.randint(0, alpha, int(m.sum()))
    return np.ascontiguousarray(t)


def _relative(rng, root, L, span, alpha):
    """L letters related to the head of root: a ragged start, about 25 % substitutions, one block of 3 - 20 letters deleted in the
    first half and one inserted in the second half of the first `span` letters -- the part the other operand shares (the path
    leaves the diagonal: the recursion's windows are unequal)"""
    s = root[rng.randint(1, 5):][:L + 24].copy()
    m = rng.rand(len(s)) < 0.25
    s[m] = rng.randint(0, alpha, int(m.sum()))
    if span >= 48:
        d, i = (int(x) for x in rng.randint(3, 21, 2))
        p = rng.randint(span // 8, span // 2 - d)
        s = np.concatenate([s[:p], s[p + d:]])
        q = rng.randint(span // 2, span - span // 8 - i)
        s = np.concatenate([s[:q], rng.randint(0, alpha, i).astype(np.uint8), s[q:]])
    assert len(s) >= L
    return np.ascontiguousarray(s[:L])


@functools.lru_cache(maxsize=None)
def job(kind, rows, cols, alphabet):
    """(codes, tasks, seq_distances) -- the root is the last task"""
    rng = np.random.RandomState(seed_of(kind, rows, cols, alphabet))
    alpha = 4 if alphabet == "dna" else 20
    root = rng.randint(0, alpha, max(rows, cols) + 64).astype(np.uint8)
    a = np.ascontiguousarray(root[:rows])
    b = _relative(rng, root, cols, min(rows, cols), alpha)
    if kind == "ss":
        codes, tasks = [a, b], [(0, 1, 2)]
    elif kind == "pp":
        codes, tasks = [a, _copy(rng, a, alpha), b, _copy(rng, b, alpha)], [(0, 1, 4), (2, 3, 5), (4, 5, 6)]
    else:
        codes, tasks = [a, _copy(rng, a, alpha), b], [(0, 1, 3), (3, 2, 4) if kind == "sp" else (2, 3, 4)]
    if alphabet == "bzx":
        codes = [c.copy() for c in codes]
        for c in codes:
            idx = rng.randint(0, len(c), max(len(c) // 50, 1))
            c[idx] = rng.randint(20, 23, len(idx)).astype(np.uint8)
    for c in codes:
        c.setflags(write=False)
    return codes, np.array(tasks, np.int32), np.linspace(0.2, 1.1, len(codes)).astype(np.float32)


def intended_root(kind, rows, cols):
    """(len_a, len_b, kind, swapped) of the root's record.  Seq-seq and profile-profile: the rows are the shorter operand and
    equal lengths swap; seq-profile: the rows are the profile, a sequence as operand a is a swap."""
    if kind == "sp_mirror":
        return cols, rows, SP, 1
    if kind == "sp":
        return rows, cols, SP, 0
    return rows, cols, SS if kind == "ss" else PP, int(rows == cols)


def strips_of(nrows, srows):
    """ka_strips_of (ka_pass.h)"""
    return 1 if nrows <= 0 else (nrows + srows - 1) // srows


def passes(la):
    """rows of a task's top-level forward and backward pass"""
    return la // 2, la - la // 2


def last_strip_rows(nrows, srows):
    """`nr` of a pass's last strip (ka_strip: min(SROWS, nrows - u0)); 0 for the empty pass"""
    return nrows - (strips_of(nrows, srows) - 1) * srows if nrows > 0 else 0


@functools.lru_cache(maxsize=None)
def want(kind, rows, cols, alphabet, n_anchors=0):
    """the oracle's answer: (records, coded paths, gap arrays)"""
    from oracle import oracledrv
    codes, tasks, dist = job(kind, rows, cols, alphabet)
    subm, scal = scoring(alphabet)
    if n_anchors:
        return oracledrv.msa_tree_cons(list(codes), tasks, subm, scal, dist, n_anchors, 2.0)[:3]
    return oracledrv.msa_tree(list(codes), tasks, subm, scal, dist)[:3]
