"""Writes tests/golden/col_*.npz and cal_*.npz: the column correctness and the calibration metrics of the reference's
benchmarks/downstream/calibration.py (_column_correctness, brier_score, expected_calibration_error, calibration_curve) and
mask_alignment_by_confidence of its benchmarks/downstream/utils.py.  Needs the reference's sources and no GPU:

    python tests/golden/make_golden_correctness.py [REFERENCE_ROOT]        (default: $KALIGN_REF or /root/reference)

The two files are loaded by path (nothing else of the reference is imported).  The files written hold data only:
    col_<case>.npz   correct  uint8 [K, W]: _column_correctness of each of the K tests of cmp_<case>.npz against its
                     reference, sequences matched by name.  The rows are not stored again: a test reads them from the cmp_ file.
    cal_<name>.npz   predicted float64 [n], actual uint8 [n], seg_first int64 [S + 1], n_bins int64; per slot (the S segments,
                     then the pool of all items in order): brier float64 [S + 1], ece float64 [S + 1], fraction float64
                     [S + 1, n_bins] (NaN: empty bin), counts int64 [S + 1, n_bins]; centers float64 [n_bins].
    cal_ens_<src>.npz  also hold mask_alignment_by_confidence of the ensemble's rows: rows uint8 [N, W], conf float32 [W],
                     mask_thr float64 [k], mask_w int64 [k] (columns retained), mask_rows uint8: the N rows of a threshold
                     back to back, thresholds in order.
"""
import glob
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def load(root, name):
    path = os.path.join(root, "benchmarks", "downstream", name + ".py")
    spec = importlib.util.spec_from_file_location("kalign_downstream_" + name, path)
    m = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = m                     # (dataclasses looks its module up)
    spec.loader.exec_module(m)
    return m


def metrics(cal, predicted, actual, seg_first, n_bins):
    """the reference's three functions per segment and on the pool, on plain Python lists as it takes them"""
    p = [float(x) for x in predicted]
    a = [int(x) for x in actual]
    S = len(seg_first) - 1
    slots = [(int(seg_first[s]), int(seg_first[s + 1])) for s in range(S)] + [(0, len(p))]
    brier, ece = np.zeros(S + 1), np.zeros(S + 1)
    frac, counts = np.zeros((S + 1, n_bins)), np.zeros((S + 1, n_bins), np.int64)
    centers = None
    for s, (lo, hi) in enumerate(slots):
        brier[s] = cal.brier_score(p[lo:hi], a[lo:hi])
        ece[s] = cal.expected_calibration_error(p[lo:hi], a[lo:hi], n_bins)
        centers, f, c = cal.calibration_curve(p[lo:hi], a[lo:hi], n_bins)
        frac[s], counts[s] = f, c
    return dict(predicted=np.asarray(p, np.float64), actual=np.asarray(a, np.uint8), seg_first=np.asarray(seg_first, np.int64),
                n_bins=np.int64(n_bins), brier=brier, ece=ece, fraction=frac, counts=counts, centers=np.asarray(centers, np.float64))


def save(name, **kw):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **kw)
    assert os.path.getsize(path) < 100 * 1000, (name, os.path.getsize(path))
    print("%-28s %6d bytes" % (name, os.path.getsize(path)))


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("KALIGN_REF", "/root/reference")
    cal, utils = load(root, "calibration"), load(root, "utils")
    # ---- col_*: every stored (reference, test) pair ----
    flags = []
    for src in sorted(glob.glob(os.path.join(HERE, "cmp_*.npz"))):
        name = os.path.basename(src)[4:-4]
        z = np.load(src)
        names = [str(n) for n in z["names"]]
        tnames = [str(n) for n in z["test_names"]] if "test_names" in z.files else names
        ref = [str(r) for r in z["ref"]]
        out = [cal._column_correctness([str(r) for r in t], ref, tnames, names) for t in z["tests"]]
        flags.extend(out)
        save("col_" + name, correct=np.asarray(out, np.uint8))
    assert len(flags) == 28
    # ---- cal_*: the real ensembles' column confidences against the correctness of their rows versus member 0 ----
    for src in ("bb11001_r3", "bb30014_r3", "dna40_r3"):
        z = np.load(os.path.join(HERE, "ens_real_%s.npz" % src))
        rows, m0 = [str(r) for r in z["ens_rows"]], [str(r) for r in z["members"][0]]
        names = ["s%d" % i for i in range(len(rows))]
        conf = z["ens_col_conf"]
        assert conf.dtype == np.float32 and len(conf) == len(rows[0])
        kw = metrics(cal, conf, cal._column_correctness(rows, m0, names, names), [0, len(conf)], 10)
        # thresholds at, just above and just below values that occur (the comparison is in double), and the ends
        v = float(np.sort(np.unique(conf))[len(np.unique(conf)) // 2])
        thr = [0.0, 0.5, v, float(np.nextafter(v, 2.0)), float(np.nextafter(v, -1.0)), 2.0 / 3.0, 1.0]
        w, kept = [], []
        for t in thr:
            masked, n = utils.mask_alignment_by_confidence(rows, [float(x) for x in conf], t)
            w.append(n)
            kept.append(np.frombuffer("".join(masked).encode("latin-1"), np.uint8))
        save("cal_ens_" + src, rows=np.frombuffer("".join(rows).encode("latin-1"), np.uint8).reshape(len(rows), -1), conf=conf,
             mask_thr=np.asarray(thr, np.float64), mask_w=np.asarray(w, np.int64), mask_rows=np.concatenate(kept), **kw)
    # ---- seeded random predictions (float32 values widened) against the flags of col_*, a segment per pair ----
    rng = np.random.default_rng(20261020)
    actual = np.concatenate([np.asarray(f, np.uint8) for f in flags])
    seg_first = np.concatenate([[0], np.cumsum([len(f) for f in flags])])
    pred = rng.random(len(actual), dtype=np.float32).astype(np.float64)
    save("cal_random10", **metrics(cal, pred, actual, seg_first, 10))
    save("cal_random7", **metrics(cal, pred, actual, seg_first, 7))
    # ---- predictions exactly at 0.0, k / 10 and 1.0 ----
    exact = [0.0] + [k / 10 for k in range(1, 10)] + [1.0]
    pred = np.asarray(exact * 6, np.float64)
    act = (np.arange(len(pred)) * 7 % 3 == 0).astype(np.uint8)
    save("cal_exact10", **metrics(cal, pred, act, [0, 11, 33, len(pred)], 10))
    save("cal_exact7", **metrics(cal, pred, act, [0, 11, 33, len(pred)], 7))
    # ---- all items in one bin; an empty segment (and an empty first and last one) ----
    pred = 0.55 + 0.04 * rng.random(40)
    act = (rng.random(40) < 0.6).astype(np.uint8)
    save("cal_onebin", **metrics(cal, pred, act, [0, 40], 10))
    pred = rng.random(23)
    act = (rng.random(23) < pred).astype(np.uint8)
    save("cal_empty_segment", **metrics(cal, pred, act, [0, 0, 9, 9, 23, 23], 10))
    save("cal_no_items", **metrics(cal, [], [], [0, 0], 7))


if __name__ == "__main__":
    main()
