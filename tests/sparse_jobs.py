"""Designed jobs for the gathered profile-profile dot product (ka_pass.h: KA_SPARSE_NT): shared by tests/test_gpu_sparse_strips.py,
which runs them on the device, and tests/test_sparse_strip_inputs.py, which holds them on the host to what they are here for -- the
non-zero counts per row of the oracle's merged row profile, strip by strip.  Host only: nothing here imports the device library.

A job is (codes, tasks, seq_distances): a row profile R of m sequences, a column profile C of two, and the root task R x C last.
R's sequences differ by substitutions only, so R has one column per letter and the residues of a column are the letters the job put
there; R is shorter than C, so R is the operand the DP's rows run over (ka_task.h: the shorter profile).  A lane of a two-row strip
holds two neighbouring rows: its term list is the union of their residues."""
import functools
import os
import re

import numpy as np

import strip_jobs as sj

_HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=None)
def bound():
    """the compile-time bound of the gathered form, from the source: KA_SPARSE_NT"""
    src = open(os.path.join(_HERE, "..", "kalign_amd", "csrc", "ka_pass.h")).read()
    return int(re.search(r"^#define KA_SPARSE_NT (\d+)$", src, re.M).group(1))


# name -> (rows, cols): the lengths of R and C.  The kinds of job:
#   pair   R of two sequences (nsip 2 + 2): every row has one or two residues, a lane at most four -- within the bound
#   bound  R of bound + 1 identical sequences with four designed columns: exactly bound and exactly bound + 1 distinct residues in
#          neighbouring strips of either top-level pass
#   narrow nsip 2 + 2; R starts with a block C lacks and C ends with a tail R lacks (terminal gaps both): below the top level the
#          recursion's first window has 140-row passes over fewer columns than a strip has lanes
PAIR = {
    "rows70": (70, 96), "rows150": (150, 176), "rows300": (300, 330), "bzx150": (150, 176), "bzx300": (300, 330),
    "narrow": (560, 580),
}
BOUND_ROWS, BOUND_COLS = 300, 330
# designed columns of a bound job: (column of R, distinct residues relative to the bound).  Rows 0 .. 149 are the forward pass
# (strips of rows 0 .. 127 and 128 .. 149), rows 299 .. 150 the backward pass (strips of rows 299 .. 172 and 171 .. 150).
BOUND_COLUMNS = [(40, 0), (140, 1), (250, 0), (160, 1)]
NARROW_BLOCK = 260


def pair_names():
    return list(PAIR)


def bound_names():
    return ["bound"]


def _seed(name):
    return 700000 + sum((i + 1) * ord(ch) for i, ch in enumerate(name))


def _freeze(codes):
    for c in codes:
        c.setflags(write=False)
    return codes


@functools.lru_cache(maxsize=None)
def job(name):
    rng = np.random.RandomState(_seed(name))
    if name in PAIR:
        rows, cols = PAIR[name]
        if name == "narrow":
            shared = rng.randint(0, 20, rows - NARROW_BLOCK).astype(np.uint8)
            a = np.concatenate([rng.randint(0, 20, NARROW_BLOCK).astype(np.uint8), shared])
            b = np.concatenate([shared, rng.randint(0, 20, cols - len(shared)).astype(np.uint8)])
        else:
            root = rng.randint(0, 20, cols + 64).astype(np.uint8)
            a = np.ascontiguousarray(root[:rows])
            b = sj._relative(rng, root, cols, rows, 20)
        codes = [a, sj._copy(rng, a, 20), b, sj._copy(rng, b, 20)]
        if name.startswith("bzx"):
            codes = [c.copy() for c in codes]
            for c in codes:
                idx = rng.randint(0, len(c), max(len(c) // 25, 1))
                c[idx] = rng.randint(20, 23, len(idx)).astype(np.uint8)
        tasks = [(0, 1, 4), (2, 3, 5), (4, 5, 6)]
    else:
        b_ = bound()
        m = b_ + 1
        root = rng.randint(0, 20, BOUND_COLS + 64).astype(np.uint8)
        base = root[:BOUND_ROWS].copy()
        for col, _ in BOUND_COLUMNS:                      # (both neighbours of a designed column hold one of its residues)
            base[col - 1] = base[col + 1] = base[col]
        rs = [base.copy() for _ in range(m)]
        for col, extra in BOUND_COLUMNS:
            for i in range(b_ + extra):
                rs[i][col] = (int(base[col]) + i) % 20
        c = sj._relative(rng, root, BOUND_COLS, BOUND_ROWS, 20)
        codes = rs + [c, sj._copy(rng, c, 20)]
        # R as a caterpillar (0, 1) -> m + 2, (m + 2, 2) -> m + 3, ...; C = (m, m + 1); the root last
        n = m + 2
        tasks, node = [(0, 1, n)], n
        for i in range(2, m):
            tasks.append((node, i, node + 1))
            node += 1
        tasks += [(m, m + 1, node + 1), (node, node + 1, node + 2)]
    codes = _freeze([np.ascontiguousarray(c) for c in codes])
    return codes, np.array(tasks, np.int32), np.linspace(0.2, 1.1, len(codes)).astype(np.float32)


def r_task(name):
    """the task that makes R (its profile is the root's row operand)"""
    return 0 if name in PAIR else bound() - 1


@functools.lru_cache(maxsize=None)
def want(name, dump_task=-1):
    """the oracle's answer: (records, coded paths, gap arrays, the dumped profile of dump_task's node or None)"""
    from oracle import oracledrv
    codes, tasks, dist = job(name)
    subm, scal = sj.scoring("protein")
    return oracledrv.msa_tree(list(codes), tasks, subm, scal, dist, dump_task=dump_task)


def strip_terms(residues, srows=128):
    """residues: per row of R the set of residues with a non-zero count.  For the root's forward and backward top-level pass the
    list, strip by strip, of the longest term list among the strip's lanes (two rows per lane: ka_strip, Q = 2)."""
    la = len(residues)
    mid = la // 2
    out = []
    for rows in (list(range(0, mid)), list(range(la - 1, mid - 1, -1))):
        per = []
        for u0 in range(0, len(rows), srows):
            strip = rows[u0:u0 + srows]
            per.append(max(len(residues[strip[i]] | (residues[strip[i + 1]] if i + 1 < len(strip) else set())) for i in range(0, len(strip), 2)))
        out.append(per)
    return out
