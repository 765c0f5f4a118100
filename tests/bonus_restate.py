"""A plain-numpy restatement of anchor_consistency_get_bonus_profile for seq-seq tasks, over position maps.

For a task whose operands are both single sequences a DP row's bonus cells follow from the two sequences' position maps
alone (a member's confidence is 1): anchor k adds weight / K to cell (i, j) when row residue i and column residue j lie on
the same position of anchor k.  Of several column residues on one anchor position the LAST one wins (the inverse map is
filled in column order); hits of several anchors in one cell are ONE entry, summed in anchor order; and the forward pass's
1-based column reaches, in a row's last column, flat index i * cols + cols: row i + 1's cell at column 0, the row's
wrap-around entry.  Rows and columns follow the DP operands (the shorter sequence gives the rows; ties swap).

entries() returns the rows' entry lists; stats() counts the states of the lists that the streamed-bonus kernels
(more than five anchors) exist for.  tests/test_stream_bonus_inputs.py holds the seeded jobs of
tests/test_gpu_stream_bonus.py to them.  Measured there (seq-seq tasks only; `longest` / `> 5` count a row's distinct
bonus columns without the wrap-around entry):

    job                    rows  longest  > 5 cols  no entry  summed cell  wrap-around
    boundary K = 6          557        6        10         0          411           14
    boundary K = 10         331       10        95         1          309           11
    boundary K = 11         486        8        19         4          276           35
    boundary K = 21         501       11       143         4          422           66
    boundary K = 33         486       13       259         0          456           82
    K = 128, nucleotides   1914       25      1833         0         1905          800
    K = 128, protein       1878       26      1866         0         1878          412
    refinement, K = 11      299        7        30         2          281           14

The eight-sequence window shapes (stream_jobs.shape_job, K = 8) add 26 one-row tasks and lists of up to seven columns.
"""
import numpy as np


def seq_seq_tasks(tasks, n):
    return [t for t, (a, b, _) in enumerate(np.asarray(tasks)) if a < n and b < n]


def entries(maps, lens, a, b, weight=2.0):
    """Row lists of the seq-seq task (a, b): a list per DP row of (column, float32 value, anchors that hit the cell),
    ascending by column; the wrap-around entry has column == cols.  Returns (rows, cols, lists)."""
    K = len(maps[a])
    swapped = not (lens[a] < lens[b])
    rn, cn = (b, a) if swapped else (a, b)
    rows, cols = int(lens[rn]), int(lens[cn])
    paw = np.float32(weight) / np.float32(K)
    cells = [dict() for _ in range(rows)]
    for k in range(K):
        pr, pc = np.asarray(maps[rn][k]), np.asarray(maps[cn][k])
        inv = {}
        for j in range(cols):
            if pc[j] >= 0:
                inv[int(pc[j])] = j                              # the last column wins
        for i in range(rows):
            j = inv.get(int(pr[i])) if pr[i] >= 0 else None
            if j is None:
                continue
            val, hits = cells[i].get(j, (np.float32(0.0), 0))
            cells[i][j] = (np.float32(val + paw * np.float32(1.0) * np.float32(1.0)), hits + 1)
    out = []
    for i in range(rows):
        row = [(j, v, h) for j, (v, h) in sorted(cells[i].items())]
        if i + 1 < rows and 0 in cells[i + 1]:
            v, h = cells[i + 1][0]
            row.append((cols, v, h))
        out.append(row)
    return rows, cols, out


def stats(maps, lens, tasks, weight=2.0):
    """Counts over the rows of every seq-seq task of a job."""
    n = len(lens)
    s = dict(rows=0, longest=0, over5=0, empty=0, summed=0, wrap=0, one_row_tasks=0)
    for t in seq_seq_tasks(tasks, n):
        a, b = int(tasks[t][0]), int(tasks[t][1])
        rows, cols, lists = entries(maps, lens, a, b, weight)
        s["one_row_tasks"] += rows == 1
        for row in lists:
            plain = [e for e in row if e[0] < cols]
            s["rows"] += 1
            s["longest"] = max(s["longest"], len(plain))
            s["over5"] += len(plain) > 5
            s["empty"] += len(row) == 0
            s["summed"] += any(h > 1 for _, _, h in row)
            s["wrap"] += len(row) > len(plain)
    return s
