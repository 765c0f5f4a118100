"""A numpy / Python statement of what the gap pass of the summary stage (ka_sum_fam_gaps, ka_sum_fam_ungapped) returns for
one family, written from the stage's contract: a byte is a gap when it equals the gap byte, every other byte is a
character.  A row's record is its characters, the gap columns before its first character (leading), those after its last
(trailing) and its gap blocks, a block being a maximal run of gaps; a row without a character has leading = trailing =
width and one block.  A family's eight counts are sums of the records and the gappy columns (2 * gaps of the column > n),
its seven doubles one division each of two counts (the expansion factor: the width over the rounded mean length).  The GPU
tests hold the device to it, the host tests hold it to the goldens recorded from the reference's benchmarks/analysis.py:
compute_gap_stats (tests/golden/make_golden_gaps.py)."""
import glob
import os

import numpy as np

from sum_restate import to_array

COUNTS = ("n_seqs", "alignment_length", "characters", "total_gaps", "n_gap_blocks", "terminal_gaps", "internal_gaps", "n_gappy_columns")
VALUES = ("mean_seq_length", "expansion_factor", "gap_fraction", "mean_gap_block_len", "mean_terminal_gap", "mean_internal_gap",
          "gappy_column_fraction")
# the twelve fields of the reference's GapStats, in its order: what a golden holds
FIELDS = ("n_seqs", "alignment_length", "mean_seq_length", "expansion_factor", "total_gaps", "gap_fraction", "n_gap_blocks",
          "mean_gap_block_len", "mean_terminal_gap", "mean_internal_gap", "n_gappy_columns", "gappy_column_fraction")


def row_records(rows, gap=b"-"):
    """int32 [n, 4]: characters, leading, trailing, gap blocks of every row"""
    a = to_array(rows)
    n, w = a.shape
    g = a == gap[0]
    rec = np.zeros((n, 4), np.int32)
    for r in range(n):
        ch = np.flatnonzero(~g[r])
        rec[r, 0] = len(ch)
        rec[r, 1] = ch[0] if len(ch) else w
        rec[r, 2] = w - 1 - ch[-1] if len(ch) else w
        # a block starts at a gap that stands in column 0 or right of a character
        rec[r, 3] = int(g[r, 0]) + int((g[r, 1:] & ~g[r, :-1]).sum())
    return rec


def counts(rows, gap=b"-"):
    """the eight counts of the family, int64 [8] (COUNTS)"""
    a = to_array(rows)
    n, w = a.shape
    rec = row_records(rows, gap).astype(np.int64)
    row_gaps = w - rec[:, 0]
    col_gaps = (a == gap[0]).sum(axis=0).astype(np.int64)
    return np.array([n, w, rec[:, 0].sum(), row_gaps.sum(), rec[:, 3].sum(), (rec[:, 1] + rec[:, 2]).sum(),
                     np.maximum(0, row_gaps - rec[:, 1] - rec[:, 2]).sum(), int((2 * col_gaps > n).sum())], np.int64)


def values(c):
    """the seven doubles (VALUES) from the eight counts: Python's float division is the one IEEE division of two doubles"""
    n, w, chars, gaps, blocks, terminal, internal, gappy = (int(x) for x in c)
    mean = float(chars) / float(n) if n > 0 else 0.0
    return np.array([mean, float(w) / mean if mean > 0 else 0.0, float(gaps) / float(n * w) if n * w > 0 else 0.0,
                     float(gaps) / float(blocks) if blocks > 0 else 0.0, float(terminal) / float(n) if n > 0 else 0.0,
                     float(internal) / float(n) if n > 0 else 0.0, float(gappy) / float(w) if w > 0 else 0.0], np.float64)


def gaps(rows, gap=b"-"):
    """the dict FamilySummary.gaps() gives for the family, with its row records"""
    c = counts(rows, gap)
    d = {k: int(v) for k, v in zip(COUNTS, c)}
    d.update({k: float(v) for k, v in zip(VALUES, values(c))})
    d["gap_opens_per_seq"] = float(d["n_gap_blocks"]) / float(d["n_seqs"])
    d["rows"] = row_records(rows, gap)
    return d


def ungapped(rows, gap=b"-"):
    """the rows without their gaps, and the int64 offsets of the rows in the packed bytes"""
    rows = [r.encode("latin-1") if isinstance(r, str) else bytes(r) for r in rows]
    out = [r.replace(bytes(gap), b"") for r in rows]
    return out, np.concatenate([[0], np.cumsum([len(r) for r in out], dtype=np.int64)]).astype(np.int64)


def golden_names(golden_dir):
    """(the cases of gap_*.npz, those of gapx_*.npz), sorted"""
    return (sorted(os.path.basename(p)[4:-4] for p in glob.glob(os.path.join(golden_dir, "gap_*.npz"))),
            sorted(os.path.basename(p)[5:-4] for p in glob.glob(os.path.join(golden_dir, "gapx_*.npz"))))


def goldens(golden_dir):
    """(name, rows, the golden's twelve fields) of every recorded case: gap_<case>.npz with the rows of sum_<case>.npz,
    gapx_<case>.npz ("x <case>") with its own"""
    cases, own = golden_names(golden_dir)
    out = []
    for name in cases:
        rows = [r.tobytes() for r in np.load(os.path.join(golden_dir, "sum_%s.npz" % name))["rows"]]
        out.append((name, rows, dict(np.load(os.path.join(golden_dir, "gap_%s.npz" % name)))))
    for name in own:
        z = dict(np.load(os.path.join(golden_dir, "gapx_%s.npz" % name)))
        out.append(("x " + name, [r.tobytes() for r in z.pop("rows")], z))
    return out
