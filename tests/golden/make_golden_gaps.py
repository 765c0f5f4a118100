"""Writes tests/golden/gap_*.npz and gapx_*.npz: compute_gap_stats of the reference's benchmarks/analysis.py run on the
rows of every stored tests/golden/sum_*.npz case and on a handful of small cases of its own.  Needs the reference's sources
and no GPU:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_gaps.py [REFERENCE_ROOT]    (default: $KALIGN_REF or /root/reference)

The reference's root goes on sys.path and benchmarks.analysis is imported as a module of its package (its relative import
keeps it from being loaded by path).  The files hold data only, GapStats' twelve fields under their own names:
    n_seqs, alignment_length, total_gaps, n_gap_blocks, n_gappy_columns                        int64 []
    mean_seq_length, expansion_factor, gap_fraction, mean_gap_block_len, mean_terminal_gap,
    mean_internal_gap, gappy_column_fraction                                                   float64 []
gap_<case>.npz belongs to the `rows` of sum_<case>.npz, which are not stored again (the function gets them as str, a byte
as the latin-1 character).  gapx_<case>.npz also holds its own
    rows         uint8 [n, w]
-- an all-gap row among others, every row all-gap (mean length 0: expansion 0.0), no gap at all (no blocks: 0.0), a single
column, an even n with a column of exactly n / 2 gaps (not gappy) and one of n / 2 + 1 (gappy), rows that start, end, or
both start and end with a gap, and blocks around column 64.
"""
import dataclasses
import glob
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
INTS = ("n_seqs", "alignment_length", "total_gaps", "n_gap_blocks", "n_gappy_columns")


def own_cases():
    cases = {}

    def arr(rows):
        return np.stack([np.frombuffer(r, np.uint8) for r in rows])

    cases["allgap_row"] = arr([b"AC-GT--A", b"--------", b"-CCG--TA", b"ACCGTTTA"])
    cases["all_allgap"] = arr([b"-----", b"-----", b"-----"])
    cases["no_gap"] = arr([b"ACGTACG", b"TTGACCA"])
    cases["one_column"] = arr([b"A", b"-", b"-", b"C", b"-"])
    # four rows: column 0 holds 2 gaps (n / 2: not gappy), column 1 holds 3 (gappy), column 2 holds 4, column 3 holds 1
    cases["half_columns"] = arr([b"---A", b"---C", b"AC-G", b"C---"])
    cases["ends"] = arr([b"--ACGT", b"ACGT--", b"-AC-G-", b"A----C", b"-A-C-G", b"ACGTAC"])
    rng = np.random.default_rng(20261020)
    a = rng.choice(np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8), size=(6, 131))
    a[0, 60:64] = ord("-")                                       # a block that ends at column 63
    a[1, 64:70] = ord("-")                                       # ... starts at column 64
    a[2, 62:66] = ord("-")                                       # ... crosses the edge
    a[3, 63] = ord("-")                                          # lone gaps on either side of it
    a[4, 64] = ord("-")
    a[5, :] = ord("-")
    a[5, 63] = ord("A")                                          # lone characters on either side of it
    a[4, 100:] = ord("-")
    a[4, 130] = ord("K")
    cases["edge64"] = a
    return cases


def record(an, a):
    st = an.compute_gap_stats({"s%d" % i: bytes(r).decode("latin-1") for i, r in enumerate(a)})
    d = dataclasses.asdict(st)
    assert len(d) == 12
    return {k: np.array(v, np.int64 if k in INTS else np.float64) for k, v in d.items()}


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("KALIGN_REF", "/root/reference")
    sys.dont_write_bytecode = True
    sys.path.insert(0, root)
    import benchmarks.analysis as an

    def write(path, name, a, **more):
        np.savez_compressed(path, **record(an, a), **more)
        assert os.path.getsize(path) < 100 * 1000, (name, os.path.getsize(path))
        print("%-28s %3d x %4d  %6d bytes" % (name, a.shape[0], a.shape[1], os.path.getsize(path)))

    for src in sorted(glob.glob(os.path.join(HERE, "sum_*.npz"))):
        name = os.path.basename(src)[4:-4]
        write(os.path.join(HERE, "gap_%s.npz" % name), name, np.load(src)["rows"])
    for name, a in own_cases().items():
        write(os.path.join(HERE, "gapx_%s.npz" % name), "x " + name, a, rows=a.astype(np.uint8))


if __name__ == "__main__":
    main()
