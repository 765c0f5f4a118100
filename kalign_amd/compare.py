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
