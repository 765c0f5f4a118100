"""Writes tests/golden/sum_*.npz: python-kalign's kalign.utils (alignment_stats, consensus_sequence, remove_gap_columns,
trim_alignment) run on stored and seeded alignments.  Needs the reference's sources and no GPU:

    python tests/golden/make_golden_summary.py [REFERENCE_ROOT]        (default: $KALIGN_REF or /root/reference)

utils.py is loaded by path (the package itself needs its compiled extension).  Per case the file holds data only:
    rows         uint8 [n, w]: the alignment (the utilities get it as str, a byte as the latin-1 character)
    stats_i      int64 [2]: length, n_sequences;   stats_f  float64 [3]: gap_fraction, conservation, identity
    cons_thr     float64 [5];  cons  uint8 [5, w]: consensus_sequence at each threshold
    rg_thr       float64 [5];  rg_w  int64 [5];  rg  uint8: remove_gap_columns at each threshold, the n rows of a
                 threshold back to back, thresholds in order
    trim_arg     int64 [k, 2], trim_none  bool [k, 2] (start / end given as None);  trim_w  int64 [k];  trim  uint8: as rg

Sources: the reference rows of a few tests/golden/cmp_*.npz cases, and seeded edge cases: one row, an all-gap column and
an all-gap row, three-way ties won by a character first seen in the last rows, upper and lower case of one letter in one
column, '.' and '*', the bytes 0x01, 0x80 and 0xFF, a DNA-only family and the same with one 'X'.
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CONS_THR = np.array([0.0, 0.34, 0.5, 2.0 / 3.0, 1.0])
RG_THR = np.array([0.0, 0.25, 1.0 / 3.0, 0.5, 1.0])
STORED = ["cmp_BB12006", "cmp_prot32x200", "cmp_dna16x300_rev", "cmp_ens_bb30014_r3_0", "cmp_ens_dna40_r3_1", "cmp_syn_lower", "cmp_syn_n2",
          "cmp_syn_gapfrac5", "cmp_ens_bb11001_r8_0"]


def load_utils(root):
    spec = importlib.util.spec_from_file_location("kalign_utils_ref", os.path.join(root, "python-kalign", "utils.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def trims(w):
    """(start, end) pairs the reference accepts at width w"""
    cand = [(None, None), (1, None), (None, -1), (-3, None), (w // 3, 2 * w // 3 + 1), (-10 ** 6, 2), (w - 1, 10 ** 6), (0, 1)]
    out = []
    for s, e in cand:
        s2 = 0 if s is None else max(0, w + s) if s < 0 else s
        e2 = w if e is None else max(0, w + e) if e < 0 else e
        if s2 < e2:
            out.append((s, e))
    return out


def seeded_cases():
    rng = np.random.default_rng(20261019)
    cases = {}

    def rand(n, w, alphabet, gap_p):
        a = rng.choice(np.frombuffer(alphabet, np.uint8), size=(n, w))
        a[rng.random((n, w)) < gap_p] = ord("-")
        return a

    cases["one_row"] = rand(1, 37, b"ACGT", 0.2)
    a = rand(7, 66, b"ACDEFGHIKLMNPQRSTVWY", 0.3)
    a[:, 5] = ord("-")
    a[:, 65] = ord("-")
    a[3, :] = ord("-")
    cases["allgap_col_row"] = a
    # three-way ties: rows 0..2 hold singletons that lose, the three tied characters appear from row 3 on, the winner
    # (first seen) differs by column; the last column's winner is first seen in the last rows
    a = np.full((9, 5), ord("-"), np.uint8)
    a[:, 0] = np.frombuffer(b"QRSAABBCC", np.uint8)
    a[:, 1] = np.frombuffer(b"QRSCCBBAA", np.uint8)
    a[:, 2] = np.frombuffer(b"---BCABCA", np.uint8)
    a[:, 3] = np.frombuffer(b"Q-R-TUTUV", np.uint8)
    a[:, 4] = np.frombuffer(b"Q--zyxxyz", np.uint8)
    cases["ties"] = a
    a = rand(6, 40, b"Aa", 0.15)
    a[:, 0] = np.frombuffer(b"AaAaAa", np.uint8)
    a[:, 1] = np.frombuffer(b"aAAa-a", np.uint8)
    cases["case"] = a
    cases["dots_stars"] = rand(8, 70, b"AC.*GT", 0.2)
    a = rand(5, 130, b"ACGU", 0.25)
    a[1, 3] = 0x01
    a[2, 3] = 0x01
    a[0, 64] = 0x80
    a[4, 64] = 0x80
    a[3, 129] = 0xFF
    cases["bytes"] = a
    a = rand(12, 129, b"ACGTacgtNU", 0.2)
    cases["dna_only"] = a
    b = a.copy()
    b[7, 100] = ord("X")
    cases["dna_one_x"] = b
    cases["wide_shallow"] = rand(3, 257, b"ACDEFGHIKLMNPQRSTVWY", 0.4)
    cases["deep_narrow"] = rand(65, 9, b"ACGT", 0.5)
    return cases


def record(u, a):
    rows = [bytes(r).decode("latin-1") for r in a]
    n, w = a.shape
    st = u.alignment_stats(rows)
    out = dict(rows=a.astype(np.uint8), stats_i=np.array([st["length"], st["n_sequences"]], np.int64),
               stats_f=np.array([st["gap_fraction"], st["conservation"], st["identity"]], np.float64), cons_thr=CONS_THR, rg_thr=RG_THR)
    out["cons"] = np.stack([np.frombuffer(u.consensus_sequence(rows, float(t)).encode("latin-1"), np.uint8) for t in CONS_THR])
    assert out["cons"].shape == (len(CONS_THR), w)
    rg = [u.remove_gap_columns(rows, float(t)) for t in RG_THR]
    out["rg_w"] = np.array([len(r[0]) for r in rg], np.int64)
    out["rg"] = np.frombuffer("".join("".join(r) for r in rg).encode("latin-1"), np.uint8)
    tr = trims(w)
    got = [u.trim_alignment(rows, s, e) for s, e in tr]
    out["trim_arg"] = np.array([[0 if s is None else s, 0 if e is None else e] for s, e in tr], np.int64)
    out["trim_none"] = np.array([[s is None, e is None] for s, e in tr], bool)
    out["trim_w"] = np.array([len(r[0]) for r in got], np.int64)
    out["trim"] = np.frombuffer("".join("".join(r) for r in got).encode("latin-1"), np.uint8)
    return out


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("KALIGN_REF", "/root/reference")
    u = load_utils(root)
    cases = {}
    for name in STORED:
        z = np.load(os.path.join(HERE, name + ".npz"))
        cases[name[4:]] = np.stack([np.frombuffer(str(r).encode(), np.uint8) for r in z["ref"]])
    cases.update(seeded_cases())
    for name, a in cases.items():
        path = os.path.join(HERE, "sum_%s.npz" % name)
        np.savez_compressed(path, **record(u, a))
        assert os.path.getsize(path) < 100 * 1000, (name, os.path.getsize(path))
        print("%-28s %3d x %4d  %6d bytes" % (name, a.shape[0], a.shape[1], os.path.getsize(path)))


if __name__ == "__main__":
    main()
