"""Scoring an alignment against a reference alignment: kalign_msa_compare (SP) and kalign_msa_compare_detailed /
_with_mask (POAR recall, precision, F1, TC; lib/src/msa_cmp.c) on the device (Context.comparer).

The reference pairs the rows of the two alignments after sorting both by name (kalign_sort_msa) and refuses a name that
occurs twice (kalign_check_msa).  compare() does the same with named rows; rows without names are paired by position.  compare_families() does it for
a batch of families, each with its own reference, in one device pass (Context.family_comparer)."""
from .api import KalignAmdError
from .synth import read_fasta


def _named(aln, what):
    """{name: row} / [(name, row)] -> rows sorted by name (bytes order, as strncmp), names; a plain row list -> rows, None"""
    if isinstance(aln, dict):
        items = list(aln.items())
    else:
        items = list(aln)
        if not items or not isinstance(items[0], tuple):
            return [x.encode() if isinstance(x, str) else bytes(x) for x in items], None
    names = [n.encode() if isinstance(n, str) else bytes(n) for n, _ in items]
    seen = set()
    for n in names:
        if n in seen:
            raise KalignAmdError("%s alignment: the name %r occurs twice" % (what, n.decode(errors="replace")))
        seen.add(n)
    order = sorted(range(len(items)), key=lambda k: names[k])
    rows = [items[k][1] for k in order]
    return [x.encode() if isinstance(x, str) else bytes(x) for x in rows], [names[k] for k in order]


def pair_rows(ref, test):
    """the two alignments' rows in the reference's pairing: sorted by name when named (both must then hold the same
    names), by position otherwise.  Returns (ref_rows, test_rows)."""
    r, rn = _named(ref, "reference")
    t, tn = _named(test, "test")
    if (rn is None) != (tn is None):
        raise KalignAmdError("one alignment has names and the other has none")
    if len(r) != len(t):
        raise KalignAmdError("the reference has %d sequences, the test alignment %d" % (len(r), len(t)))
    if rn is not None and rn != tn:
        missing = sorted(set(rn) - set(tn)) or sorted(set(tn) - set(rn))
        raise KalignAmdError("the alignments do not hold the same names (%r is in one only)" % missing[0].decode(errors="replace"))
    return r, t


def compare(ctx, ref, test, max_gap_frac=-1.0, column_mask=None):
    """test scored against ref on ctx's device.  ref / test: lists of rows (paired by position), lists of (name, row) or
    {name: row} (paired by name).  column_mask (one int per reference column) as kalign_msa_compare_with_mask, else
    max_gap_frac as kalign_msa_compare_detailed.  Returns Comparer.score's dict: sp (kalign_msa_compare's float), recall,
    precision, f1, tc, ref_pairs, test_pairs, common_pairs and the raw counts."""
    r, t = pair_rows(ref, test)
    cmp = ctx.comparer(r)
    try:
        return cmp.score(t, max_gap_frac=max_gap_frac, column_mask=column_mask)
    finally:
        cmp.close()


def compare_families(ctx, refs, tests, max_gap_frac=-1.0, column_masks=None):
    """compare() for a batch of families in one device pass (Context.family_comparer): refs[f] / tests[f] as compare()
    takes ref / test, each family's rows paired as pair_rows pairs them; max_gap_frac one value or one per family,
    column_masks None or per family None or a mask.  Returns one compare() dict per family; an error names the family."""
    refs, tests = list(refs), list(tests)
    if len(refs) != len(tests):
        raise KalignAmdError("%d reference alignments, %d test alignments" % (len(refs), len(tests)))
    r, t = [], []
    for f, (a, b) in enumerate(zip(refs, tests)):
        try:
            ra, tb = pair_rows(a, b)
        except KalignAmdError as e:
            raise KalignAmdError("family %d: %s" % (f, e)) from None
        r.append(ra)
        t.append(tb)
    cmp = ctx.family_comparer(r)
    try:
        return cmp.score(t, max_gap_frac=max_gap_frac, column_masks=column_masks)
    finally:
        cmp.close()


def compare_files(ctx, ref_path, test_path, max_gap_frac=0.2, column_mask=None):
    """compare() of two aligned FASTA files, rows paired by name (python-kalign's compare_detailed default: 0.2)"""
    rn, rs = read_fasta(ref_path)
    tn, ts = read_fasta(test_path)
    return compare(ctx, list(zip(rn, rs)), list(zip(tn, ts)), max_gap_frac=max_gap_frac, column_mask=column_mask)


# ---- where a test alignment is right: column correctness and the calibration of confidences ----
# (_column_correctness, brier_score, expected_calibration_error, calibration_curve of the reference's
# benchmarks/downstream/calibration.py; the flags come from the device, the metrics are host arithmetic in the library)
def _paired_families(refs, tests):
    refs, tests = list(refs), list(tests)
    if len(refs) != len(tests):
        raise KalignAmdError("%d reference alignments, %d test alignments" % (len(refs), len(tests)))
    r, t = [], []
    for f, (a, b) in enumerate(zip(refs, tests)):
        try:
            ra, tb = pair_rows(a, b)
        except KalignAmdError as e:
            raise KalignAmdError("family %d: %s" % (f, e)) from None
        r.append(ra)
        t.append(tb)
    return r, t


def column_correctness_families(ctx, refs, tests):
    """_column_correctness for a batch of families in one device pass (FamilyComparer.detail): per family the uint8 flag
    of every test column -- 1 when its residues (none or one: 1) all lie in one column of the family's reference.  refs /
    tests as compare_families() takes them; a column's flag does not depend on the order of the rows."""
    r, t = _paired_families(refs, tests)
    cmp = ctx.family_comparer(r)
    try:
        return [d["test_columns"]["correct"] for d in cmp.detail(t)]
    finally:
        cmp.close()


def column_correctness(ctx, ref, test):
    """_column_correctness of one test alignment against its reference (true) alignment: one uint8 flag per test column"""
    return column_correctness_families(ctx, [ref], [test])[0]


def calibration(predicted, actual, n_bins=10, segments=None):
    """brier_score, expected_calibration_error and calibration_curve of (predicted confidence, actual 0 / 1) items, with
    the reference's arithmetic (ka_calibration; host only).  Returns a dict with the reference's keys: brier_score, ece,
    bin_centers, fraction_correct (NaN for an empty bin), bin_counts.  With segments (the number of items of each segment,
    in order) returns (one such dict per segment, the dict of the pool of all items in order)."""
    import ctypes as C

    import numpy as np

    from .api import _ptr, load_library
    L = load_library()
    p = np.ascontiguousarray(predicted, np.float64).reshape(-1)
    a = np.asarray(actual).reshape(-1)
    if len(a) != len(p):
        raise KalignAmdError("%d predicted values, %d actual values" % (len(p), len(a)))
    if len(a) and (a != (a != 0)).any():
        k = int(np.flatnonzero(a != (a != 0))[0])
        raise KalignAmdError("ka_calibration: item %d: actual %s is neither 0 nor 1" % (k, a[k]))
    a = np.ascontiguousarray(a, np.uint8)
    sizes = [len(p)] if segments is None else [int(n) for n in segments]
    if any(n < 0 for n in sizes) or sum(sizes) != len(p):
        raise KalignAmdError("the segments hold %d items, %d are given" % (sum(sizes), len(p)))
    first = np.concatenate([[0], np.cumsum(sizes, dtype=np.int64)]).astype(np.int64)
    S = len(sizes) + 1
    nb = max(int(n_bins), 0)
    brier, ece = np.zeros(S, np.float64), np.zeros(S, np.float64)
    frac, counts = np.zeros((S, nb), np.float64), np.zeros((S, nb), np.int64)
    if L.ka_calibration(len(sizes), _ptr(first), _ptr(p), _ptr(a), C.c_int(int(n_bins)), _ptr(brier), _ptr(ece), _ptr(frac), _ptr(counts)) != 0:
        raise KalignAmdError(L.ka_last_error().decode())
    width = 1.0 / n_bins
    centers = [(b + 0.5) * width for b in range(n_bins)]
    out = [dict(brier_score=float(brier[s]), ece=float(ece[s]), bin_centers=list(centers), fraction_correct=frac[s].tolist(),
                bin_counts=[int(x) for x in counts[s]]) for s in range(S)]
    return out[-1] if segments is None else (out[:-1], out[-1])


def calibrate_families(ctx, refs, tests, column_confidences, n_bins=10):
    """the calibration of per-column confidences (FamilyEnsemble.confidence's column values) against the column
    correctness of the test alignments: column_confidences[f] one value per test column of family f.  Returns
    dict(correct=the flags per family, families=calibration() per family, pooled=calibration() of all columns, families in
    order)."""
    import numpy as np
    flags = column_correctness_families(ctx, refs, tests)
    conf = [np.asarray(c, np.float64).reshape(-1) for c in column_confidences]
    if len(conf) != len(flags):
        raise KalignAmdError("%d confidence arrays for %d families" % (len(conf), len(flags)))
    for f, (c, g) in enumerate(zip(conf, flags)):
        if len(c) != len(g):
            raise KalignAmdError("family %d: %d confidences for %d test columns" % (f, len(c), len(g)))
    per, pooled = calibration(np.concatenate(conf) if conf else [], np.concatenate(flags) if flags else [], n_bins, [len(g) for g in flags])
    return dict(correct=flags, families=per, pooled=pooled)
