"""A numpy statement of what the summary stage (ka_sum_fam) returns for one family, written from the stage's contract:
the rule for a byte, the five per-column values, the six counts and three doubles of a family, the consensus, the kept
columns and the compacted rows.  The GPU tests hold the device to it, the host tests hold it to the goldens recorded from
python-kalign's kalign.utils (tests/golden/make_golden_summary.py)."""
import numpy as np


def to_array(rows):
    """rows (bytes / str, one length) -> uint8 [n, width]"""
    rows = [r.encode("latin-1") if isinstance(r, str) else bytes(r) for r in rows]
    return np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), len(rows[0])).copy()


def columns(rows, gap=b"-"):
    """per column: gaps, distinct characters, the most frequent character (among equals the one first seen in the lowest
    row; the gap byte in an all-gap column) and its count, and the sum over its characters a of n_a (n_a - 1) / 2"""
    a = to_array(rows)
    g = gap[0]
    n, w = a.shape
    hist = np.zeros((w, 256), np.int64)
    for r in range(n):
        hist[np.arange(w), a[r]] += 1
    n_gap = hist[:, g].copy()
    hist[:, g] = 0
    n_distinct = (hist > 0).sum(axis=1)
    top_count = hist.max(axis=1)
    same_pairs = (hist * (hist - 1) // 2).sum(axis=1)
    # the count of every cell's byte in its column; the first row whose byte has the column's highest count
    cell = hist[np.arange(w)[None, :], a]
    first = np.argmax(cell == top_count[None, :], axis=0)
    top_char = np.where(top_count > 0, a[first, np.arange(w)], g).astype(np.uint8)
    return dict(n_gap=n_gap.astype(np.int32), n_distinct=n_distinct.astype(np.int32), top_char=top_char,
                top_count=top_count.astype(np.int32), same_pairs=same_pairs)


def summary(rows, gap=b"-"):
    """the six counts and the three doubles, each one division of two counts"""
    a = to_array(rows)
    n, w = a.shape
    c = columns(rows, gap)
    k = n - c["n_gap"].astype(np.int64)
    counts = dict(gaps=int(c["n_gap"].sum()), cells=n * w, conserved_columns=int(((k > 0) & (c["n_distinct"] == 1)).sum()), columns=w,
                  matching_pairs=int(c["same_pairs"].sum()), compared_pairs=int((k * (k - 1) // 2).sum()))
    d = dict(length=w, n_sequences=n, gap_fraction=float(counts["gaps"]) / float(counts["cells"]),
             conservation=float(counts["conserved_columns"]) / float(counts["columns"]),
             identity=float(counts["matching_pairs"]) / float(counts["compared_pairs"]) if counts["compared_pairs"] > 0 else 0.0)
    d.update(counts)
    return d


def ambiguous(rows, gap=b"-"):
    """b'N' when every character of the family, upper-cased (ASCII), lies in ATCGUN, else b'X'"""
    chars = set(to_array(rows).reshape(-1).tolist()) - {gap[0]}
    upper = {b - 32 if 97 <= b <= 122 else b for b in chars}
    return b"N" if upper <= set(b"ATCGUN") else b"X"


def consensus(rows, threshold=0.5, gap=b"-"):
    a = to_array(rows)
    n = a.shape[0]
    c = columns(rows, gap)
    amb = ambiguous(rows, gap)[0]
    out = bytearray()
    for col in range(a.shape[1]):
        k = n - int(c["n_gap"][col])
        if k == 0:
            out.append(gap[0])
        elif float(int(c["top_count"][col])) / float(k) >= threshold:
            out.append(int(c["top_char"][col]))
        else:
            out.append(amb)
    return bytes(out)


def keep(rows, gap_threshold=1.0, mask=None, gap=b"-"):
    """int32 0 / 1 per column: the mask (non-zero keeps) or n_gap / n < gap_threshold"""
    a = to_array(rows)
    if mask is not None:
        return (np.asarray(mask).reshape(-1) != 0).astype(np.int32)
    n = a.shape[0]
    g = columns(rows, gap)["n_gap"]
    return np.array([1 if float(int(x)) / float(n) < gap_threshold else 0 for x in g], np.int32)


def compact(rows, gap_threshold=1.0, mask=None, gap=b"-"):
    a = to_array(rows)
    kp = keep(rows, gap_threshold, mask, gap) != 0
    return [a[r, kp].tobytes() for r in range(a.shape[0])]
