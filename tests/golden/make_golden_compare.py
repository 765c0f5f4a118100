"""Writes tests/golden/cmp_*.npz: the reference's alignment comparison (kalign_msa_compare, kalign_msa_compare_detailed,
kalign_msa_compare_with_mask; lib/src/msa_cmp.c) run through oracle/_ref/libkalign_ref.so.

    python tests/golden/make_golden_compare.py        (needs oracle/_ref/libkalign_ref.so: `make -C oracle ref`)

Per case: the names, the reference rows, one or more test alignments of the same sequences, the max_gap_frac values and
a partial column mask, and per test: the SP float, and per max_gap_frac (then for the mask) the four poar doubles
(recall, precision, f1, tc) and three int64s (ref_pairs, test_pairs, common).  reference_compare() is also what
tests/test_gpu_compare.py uses for its live randomized cases; random_case() makes their alignments.

Sources: the real ensemble members of tests/golden/ens_real_*.npz scored against each other, the rows of tree goldens
against a left-packed restatement of themselves, and synthetic cases (N = 2, an all-gap column, the 1-in-5 float
boundary of max_gap_frac = 0.2, lowercase letters and '.' gaps).

The reference's reader ends the process on input it rejects (one sequence: exit status 216), so every input handed to it
here has two sequences at least, unique names, a gap somewhere and a residue in every row.
"""
import ctypes as C
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libkalign_ref.so")
FRACS = np.array([-1.0, 0.0, 0.2, 0.5, 1.0], np.float32)


class PoarScore(C.Structure):                    # struct poar_score, lib/src/msa_cmp.h
    _fields_ = [("recall", C.c_double), ("precision", C.c_double), ("f1", C.c_double), ("tc", C.c_double),
                ("ref_pairs", C.c_int64), ("test_pairs", C.c_int64), ("common", C.c_int64)]


_lib = None


def available():
    return os.path.exists(REF_SO)


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(REF_SO)
        vp = C.c_void_p
        L.kalign_read_input.argtypes = [C.c_char_p, C.POINTER(vp), C.c_int]
        L.kalign_free_msa.argtypes = [vp]
        L.kalign_free_msa.restype = None
        L.kalign_msa_compare.argtypes = [vp, vp, C.POINTER(C.c_float)]
        L.kalign_msa_compare_detailed.argtypes = [vp, vp, C.c_float, C.POINTER(PoarScore)]
        L.kalign_msa_compare_with_mask.argtypes = [vp, vp, vp, C.c_int, C.POINTER(PoarScore)]
        _lib = L
    return _lib


def _check_input(names, rows):
    assert len(rows) >= 2 and len(set(names)) == len(names), "the reference's reader needs >= 2 uniquely named rows"
    assert len(set(len(r) for r in rows)) == 1
    assert all(any(c.isascii() and c.isalpha() for c in r) for r in rows), "a row without residues"
    assert any(not (c.isascii() and c.isalpha()) for r in rows for c in r), "no gap: the reader cannot tell it is aligned"


def _read(d, tag, names, rows):
    path = os.path.join(d, tag + ".fa")
    with open(path, "w") as f:
        for n, r in zip(names, rows):
            f.write(">%s\n%s\n" % (n, r))
    m = C.c_void_p()
    assert lib().kalign_read_input(path.encode(), C.byref(m), 1) == 0, "kalign_read_input failed"
    return m


def reference_compare(names, ref_rows, test_rows, fracs=FRACS, mask=None, test_names=None):
    """the reference's three functions on (names, ref_rows) and (test_names or names, test_rows), each on freshly read
    alignments.  Returns dict(sp=float32, poar=float64[len(fracs), 4], poar_i=int64[len(fracs), 3], and with a mask
    mask_poar=float64[4], mask_i=int64[3])."""
    tn = names if test_names is None else test_names
    _check_input(names, ref_rows)
    _check_input(tn, test_rows)
    L = lib()
    d = tempfile.mkdtemp()
    out = {}
    try:
        def both():
            return _read(d, "r", names, ref_rows), _read(d, "t", tn, test_rows)

        r, t = both()
        s = C.c_float()
        assert L.kalign_msa_compare(r, t, C.byref(s)) == 0
        out["sp"] = np.float32(s.value)
        L.kalign_free_msa(r); L.kalign_free_msa(t)
        poar = np.zeros((len(fracs), 4), np.float64)
        poar_i = np.zeros((len(fracs), 3), np.int64)
        for q, fr in enumerate(fracs):
            r, t = both()
            p = PoarScore()
            assert L.kalign_msa_compare_detailed(r, t, float(fr), C.byref(p)) == 0
            poar[q] = (p.recall, p.precision, p.f1, p.tc)
            poar_i[q] = (p.ref_pairs, p.test_pairs, p.common)
            L.kalign_free_msa(r); L.kalign_free_msa(t)
        out["poar"], out["poar_i"] = poar, poar_i
        if mask is not None:
            r, t = both()
            m = np.ascontiguousarray(mask, np.int32)
            p = PoarScore()
            assert L.kalign_msa_compare_with_mask(r, t, m.ctypes.data_as(C.c_void_p), len(m), C.byref(p)) == 0
            out["mask_poar"] = np.array([p.recall, p.precision, p.f1, p.tc], np.float64)
            out["mask_i"] = np.array([p.ref_pairs, p.test_pairs, p.common], np.int64)
            L.kalign_free_msa(r); L.kalign_free_msa(t)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    return out


def random_case(rng, n, length, dna=False, gap_p=0.15, noise=0.3, width_extra=0):
    """n random sequences of about `length` residues, a random alignment of them (the reference) and a perturbed one
    (the test: each row's gaps moved with probability `noise`, `width_extra` more columns).  Returns (ref_rows,
    test_rows): str rows, every row with a residue, both with gaps."""
    alpha = np.frombuffer(b"ACGT" if dna else b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
    lens = np.maximum(1, rng.randint(int(length * 0.8), int(length * 1.2) + 1, size=n))
    seqs = [alpha[rng.randint(0, len(alpha), size=L)] for L in lens]

    def place(W, p_move):
        rows = []
        for s in seqs:
            L = len(s)
            # L residue positions among W columns: sorted random subset, then local shifts
            cols = np.sort(rng.choice(W, size=L, replace=False))
            if p_move > 0:
                for _ in range(int(p_move * L)):
                    k = rng.randint(0, L)
                    lo = cols[k - 1] + 1 if k > 0 else 0
                    hi = cols[k + 1] - 1 if k + 1 < L else W - 1
                    if hi >= lo:
                        cols[k] = rng.randint(lo, hi + 1)
            row = np.full(W, ord("-"), np.uint8)
            row[cols] = s
            rows.append(row.tobytes().decode())
        return rows

    W = int(lens.max() * (1.0 + gap_p)) + 1
    ref = place(W, 0.0)
    test = place(W + width_extra, noise) if width_extra else None
    if test is None:
        # the test: the reference's columns with some residues moved inside their free gap runs
        test = []
        for row in ref:
            b = np.frombuffer(row.encode(), np.uint8).copy()
            cols = np.flatnonzero(b != ord("-"))
            for _ in range(int(noise * len(cols))):
                k = rng.randint(0, len(cols))
                lo = cols[k - 1] + 1 if k > 0 else 0
                hi = cols[k + 1] - 1 if k + 1 < len(cols) else W - 1
                if hi >= lo:
                    nc = rng.randint(lo, hi + 1)
                    b[nc], b[cols[k]] = b[cols[k]], ord("-") if nc != cols[k] else b[cols[k]]
                    cols[k] = nc
            test.append(b.tobytes().decode())
    return ref, test


def left_packed(rows, extra=1):
    """every row's residues moved to the left, '-' after them; `extra` more columns so that the reader sees gaps"""
    W = max(sum(c.isalpha() for c in r) for r in rows) + extra
    return ["".join(c for c in r if c.isalpha()).ljust(W, "-") for r in rows]


def partial_mask(rng, W):
    m = (rng.rand(W) < 0.6).astype(np.int32)
    m[0] = 1
    return m


def write_case(name, names, ref, tests, rng, test_names=None):
    mask = partial_mask(rng, len(ref[0]))
    outs = [reference_compare(names, ref, t, mask=mask, test_names=test_names) for t in tests]
    kw = dict(names=np.array(names), ref=np.array(ref), tests=np.array(tests), fracs=FRACS, mask=mask,
              sp=np.array([o["sp"] for o in outs], np.float32), poar=np.stack([o["poar"] for o in outs]),
              poar_i=np.stack([o["poar_i"] for o in outs]), mask_poar=np.stack([o["mask_poar"] for o in outs]),
              mask_i=np.stack([o["mask_i"] for o in outs]))
    if test_names is not None:
        kw["test_names"] = np.array(test_names)
    path = os.path.join(HERE, "cmp_%s.npz" % name)
    np.savez_compressed(path, **kw)
    print("cmp_%s: %d x %d, %d tests, sp %s, %d bytes" % (name, len(ref), len(ref[0]), len(tests),
                                                          ["%.4f" % o["sp"] for o in outs], os.path.getsize(path)))


def main():
    if not available():
        sys.exit("oracle/_ref/libkalign_ref.so is missing: make -C oracle ref")
    rng = np.random.RandomState(20261016)
    # the real ensemble members: member 0 as the reference, the other members and kalign_ensemble's output as tests
    for src in ("bb11001_r8", "bb30014_r3", "dna40_r3"):
        z = np.load(os.path.join(HERE, "ens_real_%s.npz" % src))
        members = [[str(r) for r in m] for m in z["members"]]
        names = ["s%d" % i for i in range(len(members[0]))]
        tests = members[1:] + [[str(r) for r in z["ens_rows"]]]
        # the test alignments differ in width: one file per width keeps the arrays rectangular
        by_w = {}
        for t in tests:
            by_w.setdefault(len(t[0]), []).append(t)
        for q, (w, ts) in enumerate(sorted(by_w.items())):
            write_case("ens_%s_%d" % (src, q), names, members[0], ts, rng)
    # tree goldens' rows against their left-packed restatement (and the other way round)
    for src in ("tree_BB12006", "tree_prot32x200", "tree_dna16x300"):
        z = np.load(os.path.join(HERE, "%s.npz" % src))
        rows = [str(r) for r in z["rows"]]
        names = ["seq_%03d" % i for i in range(len(rows))]
        write_case("%s" % src[5:], names, rows, [left_packed(rows)], rng)
        write_case("%s_rev" % src[5:], names, left_packed(rows), [rows], rng)
    # synthetic
    ref, test = random_case(rng, 2, 60)
    write_case("syn_n2", ["b", "a"], ref, [test, ref], rng)
    ref, test = random_case(rng, 5, 40)
    # the 1-in-5 boundary of max_gap_frac = 0.2 ((float)1 / (float)5 <= 0.2f) and an all-gap column
    ref = [r[:10] + ("-" if k == 3 else "W") + r[10:] + "-" for k, r in enumerate(ref)]
    test = [r[:10] + ("-" if k == 3 else "W") + r[10:] + "-" for k, r in enumerate(test)]
    write_case("syn_gapfrac5", ["n%d" % k for k in range(5)], ref, [test], rng)
    ref, test = random_case(rng, 24, 120, noise=0.5)
    write_case("syn_prot24", ["p%02d" % k for k in range(24)], ref, [test, ref], rng)
    ref, test = random_case(rng, 16, 200, dna=True, width_extra=13, noise=0.2)
    write_case("syn_dna16_wider", ["d%02d" % k for k in range(16)], ref, [test], rng)
    ref, test = random_case(rng, 12, 80, noise=0.4)
    low = [r.lower().replace("-", ".") for r in test]
    write_case("syn_lower", ["x%02d" % k for k in range(12)], ref, [low], rng)
    # the test file in shuffled row order: the reference pairs by name
    ref, test = random_case(rng, 20, 90, noise=0.4)
    names = ["r%02d" % k for k in range(20)]
    perm = rng.permutation(20)
    write_case("syn_shuffled", names, ref, [[test[k] for k in perm]], rng, test_names=[names[k] for k in perm])


if __name__ == "__main__":
    main()
