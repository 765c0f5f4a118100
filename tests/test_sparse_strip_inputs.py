"""Host-only: the designed jobs of tests/test_gpu_sparse_strips.py (tests/sparse_jobs.py) hit the bound of the gathered dot product.

Conditions on the INPUTS, measured with the oracle: the non-zero counts per row of the merged row profile the root task reads, and
from them the longest term list of every strip of the root's two top-level passes (two rows per lane, 128-row strips) -- held
to the bound the kernel was built with (KA_SPARSE_NT in ka_pass.h).  An edit of a job, a seed or the bound cannot
quietly move the device tests off the cases they are there for."""
import numpy as np
import pytest

import sparse_jobs as sp
import strip_jobs as sj

ALL = sp.pair_names() + sp.bound_names()


def _row_profile(name):
    """(the root's record, per row of R the set of residues with a non-zero count)"""
    t = sp.r_task(name)
    recs, _, _, dump = sp.want(name, t)
    prof = dump[:64 * (recs[t].plen + 2)].reshape(-1, 64)
    return recs[len(recs) - 1], [set(np.flatnonzero(prof[r, :23]).tolist()) for r in range(1, recs[t].plen + 1)]


def test_the_bound_is_what_the_jobs_were_designed_for():
    b = sp.bound()
    assert 4 <= b <= 18                                                # (pair jobs need four terms; bound + 1 distinct residues of 20)
    codes, tasks, _ = sp.job("bound")
    assert len(codes) == b + 3 and len(tasks) == b + 2


@pytest.mark.parametrize("name", ALL)
def test_the_row_operand_is_the_designed_profile(oracle, name):
    """R has a column per letter, holding the letters of its sequences at that place; it is the root's row operand"""
    codes, tasks, _ = sp.job(name)
    root, res = _row_profile(name)
    m = 2 if name in sp.PAIR else sp.bound() + 1
    assert len(res) == len(codes[0])
    for r, s in enumerate(res):
        assert s == {int(c[r]) for c in codes[:m]}, (name, r)
    assert root.kind == sj.PP and min(root.len_a, root.len_b) == len(res) < max(root.len_a, root.len_b)
    assert (root.swapped == 0) == (root.len_a == len(res))                # (the rows are R: ka_task.h takes the shorter profile)
    assert {root.nsip_a, root.nsip_b} == {m, 2}
    if name.startswith("bzx"):
        assert any(s & {20, 21, 22} for s in res) and all(int(c.max()) >= 20 for c in codes)
    else:
        assert all(int(c.max()) <= 19 for c in codes)


@pytest.mark.parametrize("name", sp.pair_names())
def test_pair_jobs_stay_within_the_bound(oracle, name):
    """nsip 2 + 2: every strip of both top-level passes runs gathered, and has lanes whose two rows differ"""
    _, res = _row_profile(name)
    strips = sp.strip_terms(res)
    assert all(2 <= x <= sp.bound() for per in strips for x in per), (name, strips)
    rows = sp.PAIR[name][0]
    want = {70: [1, 1], 150: [1, 1], 300: [2, 2], 560: [3, 3]}[rows]      # strips per pass: a lone partial strip / a full one handing over
    assert [len(per) for per in strips] == want
    # an odd last row: its lane's row B does not exist -- the one term list a job can shorten to a single row's
    if name == "rows70":
        assert (rows // 2) % 2 == 1


def test_bound_job_puts_neighbouring_strips_either_side_of_the_bound(oracle):
    """forward pass: strip 0 exactly at the bound, strip 1 one above it; backward pass the same"""
    b, name = sp.bound(), "bound"
    _, res = _row_profile(name)
    assert sp.strip_terms(res) == [[b, b + 1], [b, b + 1]]
    # ... by the designed columns alone: every other lane holds two rows of one residue each
    designed = {c for c, _ in sp.BOUND_COLUMNS}
    assert all(len(s) == 1 for r, s in enumerate(res) if r not in designed)
    assert [len(res[c]) for c, _ in sp.BOUND_COLUMNS] == [b + e for _, e in sp.BOUND_COLUMNS]


def test_narrow_job_has_windows_with_fewer_columns_than_lanes(oracle):
    """the root's path crosses the middle row just behind R's leading block, left of column 64: the first child window of the recursion has
    280 rows (140-row passes: a full strip of 64 lanes and a partial one) over fewer than 64 columns"""
    recs, paths, _, _ = sp.want("narrow", sp.r_task("narrow"))
    r = recs[len(recs) - 1]
    assert r.swapped == 0 and r.len_a == 560
    ops = np.asarray(paths[r.path_off + 1:r.path_off + 1 + r.plen]) & 3
    # (ops of a coded path: 0 both operands advance, 1 gap in a, 2 gap in b)
    ia = np.cumsum(ops != 1)
    ib = np.cumsum(ops != 2)
    col_at_mid = int(ib[np.searchsorted(ia, 280)])
    assert 1 <= col_at_mid < 64, col_at_mid


@pytest.mark.parametrize("name", ALL)
def test_no_row_of_a_merged_profile_is_without_a_residue(oracle, name):
    """An all-gap row -- a term list of length 0 -- is not an input a task can have: every column of every profile the tree merges
    (the operands of every profile-profile task, not only the root's) holds at least one non-zero count.  The shortest list a lane
    can have is one row's own: the lane of an odd last row, whose row B lies below the strip (rows70: 35-row passes)."""
    codes, tasks, _ = sp.job(name)
    for t in range(len(tasks) - 1):
        recs, _, _, dump = sp.want(name, t)
        prof = dump[:64 * (recs[t].plen + 2)].reshape(-1, 64)
        assert (np.count_nonzero(prof[1:recs[t].plen + 1, :23], axis=1) >= 1).all(), (name, t)
