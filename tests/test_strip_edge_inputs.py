"""Host-only: the seeded jobs of tests/test_gpu_strip_edges.py (tests/strip_jobs.py) sit on the edges of the strip passes.

Conditions on the INPUTS, measured with the oracle: a later change of seeds or of the generator cannot quietly move that suite off
the strips' row and column edges.  What the device makes of a task's rows is restated here from ka_strips_of (ka_pass.h) and the
La / 2 split of a task's top level (ka_strip: r0 .. mid forwards, mid .. r1 backwards), and held to a table written out by hand."""
import numpy as np
import pytest

import strip_jobs as sj

# rows of the task -> strip height -> (strips, rows of the last strip) of the forward and of the backward top-level pass
PASSES = {
    1: {128: ((1, 0), (1, 1)), 64: ((1, 0), (1, 1))},
    2: {128: ((1, 1), (1, 1)), 64: ((1, 1), (1, 1))},
    64: {128: ((1, 32), (1, 32)), 64: ((1, 32), (1, 32))},
    127: {128: ((1, 63), (1, 64)), 64: ((1, 63), (1, 64))},
    128: {128: ((1, 64), (1, 64)), 64: ((1, 64), (1, 64))},
    129: {128: ((1, 64), (1, 65)), 64: ((1, 64), (2, 1))},
    130: {128: ((1, 65), (1, 65)), 64: ((2, 1), (2, 1))},
    255: {128: ((1, 127), (1, 128)), 64: ((2, 63), (2, 64))},
    256: {128: ((1, 128), (1, 128)), 64: ((2, 64), (2, 64))},
    257: {128: ((1, 128), (2, 1)), 64: ((2, 64), (3, 1))},
    258: {128: ((2, 1), (2, 1)), 64: ((3, 1), (3, 1))},
    259: {128: ((2, 1), (2, 2)), 64: ((3, 1), (3, 2))},
    511: {128: ((2, 127), (2, 128)), 64: ((4, 63), (4, 64))},
    512: {128: ((2, 128), (2, 128)), 64: ((4, 64), (4, 64))},
    513: {128: ((2, 128), (3, 1)), 64: ((4, 64), (5, 1))},
    514: {128: ((3, 1), (3, 1)), 64: ((5, 1), (5, 1))},
}


def _root(case):
    recs, paths, _ = sj.want(*case)
    r = recs[len(recs) - 1]
    return r, paths[r.path_off:r.path_off + r.plen + 2]


def _rows_cols(r):
    """(S.La, S.Lb) of a record, by the operand selection of ka_task.h"""
    if r.kind == sj.SP:
        return (r.len_a, r.len_b) if r.nsip_a > 1 else (r.len_b, r.len_a)
    return min(r.len_a, r.len_b), max(r.len_a, r.len_b)


def _measured():
    out = []
    for case in sj.cases():
        r, _ = _root(case)
        la, lb = _rows_cols(r)
        out.append((case, r, la, lb, {s: tuple((sj.strips_of(n, s), sj.last_strip_rows(n, s)) for n in sj.passes(la)) for s in (128, 64)}))
    return out


def test_the_table_is_the_issue_of_record():
    assert len(sj.SHAPES) == 20 and all(r <= c for r, c in sj.SHAPES)
    assert len(sj.cases()) == 3 * (20 + 20 + 24 + 24)
    assert len(sj.MODES) == 14 and len(sj.CONS_MODES) == 5 and all(m in sj.MODES for m in sj.CONS_MODES)
    assert {r for r, _ in sj.SHAPES + sj.SP_EXTRA} == set(PASSES)
    for case in sj.cases():                                            # (the generator keeps the lengths it is asked for)
        kind, rows, cols, alphabet = case
        codes, tasks, dist = sj.job(*case)
        assert [len(c) for c in codes] == {"ss": [rows, cols], "pp": [rows, rows, cols, cols]}.get(kind, [rows, rows, cols]), case
        top = max(int(c.max()) for c in codes)
        assert top <= {"protein": 19, "bzx": 22, "dna": 3}[alphabet], case
        if alphabet == "bzx":
            assert all(int(c.max()) >= 20 for c in codes), case


@pytest.mark.parametrize("case", sj.cases(), ids=sj.case_id)
def test_root_task_has_the_intended_operands(oracle, case):
    kind, rows, cols, _ = case
    r, _ = _root(case)
    assert (r.len_a, r.len_b, r.kind, r.swapped) == sj.intended_root(kind, rows, cols)
    assert _rows_cols(r) == (rows, cols)


@pytest.mark.parametrize("case", sj.cases(), ids=sj.case_id)
def test_root_task_has_the_intended_strips(oracle, case):
    r, _ = _root(case)
    la, _ = _rows_cols(r)
    for srows in (128, 64):
        got = tuple((sj.strips_of(n, srows), sj.last_strip_rows(n, srows)) for n in sj.passes(la))
        assert got == PASSES[case[1]][srows], (case, srows)


# Seq-seq from 127 rows on, as the jobs were specified; the profile jobs from 63 rows on (the sequence of 513 x 63).  The two
# shapes of one and two rows are left out (18 profile jobs).  A gap inside an operand has that operand's letters on both sides:
# with one row there is no inside.  With two rows there is one place for it, between the two letters, and such a path exists
# but is not the optimal one for these jobs: an inner gap run costs an opening that setting the two letters side by side saves.
@pytest.mark.parametrize("case", [c for c in sj.cases() if min(c[1], c[2]) >= (127 if c[0] == "ss" else 63)], ids=sj.case_id)
def test_root_path_has_a_gap_run_inside_each_operand(oracle, case):
    """not a diagonal with terminal gaps only: the recursion's windows are unequal.  (Ops of a coded path: 1 = gap in a, 2 = gap
    in b; 32 marks the terminal runs.)"""
    _, path = _root(case)
    ops = np.asarray(path[1:path[0] + 1])
    inner = ops[(ops & 32) == 0]
    assert ((inner & 3) == 1).any() and ((inner & 3) == 2).any(), case


def test_the_table_reaches_every_edge(oracle):
    m = _measured()
    per = {s: [p for _, _, _, _, by in m for p in by[s]] for s in (128, 64)}
    assert max(ns for ns, _ in per[128]) >= 3
    assert max(ns for ns, _ in per[64]) >= 5
    assert {1, 2, 127, 128} <= {last for _, last in per[128]}
    assert {1, 63, 64} <= {last for _, last in per[64]}
    # ... as the last of SEVERAL strips too (the strip that waits for a boundary row), not only as a pass of one short strip
    assert {1, 2, 127, 128} <= {last for ns, last in per[128] if ns >= 2}
    assert {1, 63, 64} <= {last for ns, last in per[64] if ns >= 2}
    cols = {lb for _, _, _, lb, _ in m}
    assert {63, 0, 1} <= {c % 64 for c in cols}
    assert {127, 0, 1} <= {c % 128 for c in cols}
    assert max(cols) > 320
    assert max(la for _, _, la, _, _ in m) >= 320
    for kind in (sj.SS, sj.SP, sj.PP):
        assert {r.swapped for _, r, _, _, _ in m if r.kind == kind} == {0, 1}, kind
    assert any(la == 1 and by[128][0] == (1, 0) for _, _, la, _, by in m)             # an empty forward pass
    # ... and every kind and alphabet meets every one of these by itself
    for kind in sj.KINDS:
        for alphabet in sj.ALPHABETS:
            mine = [x for x in m if x[0][0] == kind and x[0][3] == alphabet]
            assert {1, 2, 127, 128} <= {last for x in mine for _, last in x[4][128]}, (kind, alphabet)
            assert max(ns for x in mine for ns, _ in x[4][128]) >= 3, (kind, alphabet)
            assert {63, 0, 1} <= {x[3] % 64 for x in mine}, (kind, alphabet)
