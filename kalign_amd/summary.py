"""python-kalign's kalign.utils on the device: alignment_stats, consensus_sequence, remove_gap_columns, trim_alignment and
pairwise_identity_matrix with the reference's names, arguments and return shapes, for one alignment (a list of str) and -- in one device pass, the
number of launches independent of the batch -- for a list of families (Context.family_summary = ka_sum_fam).

gap_stats is compute_gap_stats of the reference's benchmarks/analysis.py (expansion factor, gap blocks, terminal against
internal gaps, gappy columns), dealign its dealign_msa: the sequences without their gaps.

A gap is '-'; every other character counts and is compared as it stands (upper and lower case differ), as in kalign.utils.
Results equal the reference's bit for bit.  There is no CPU fallback: every function takes a Context."""
from .api import KalignAmdError

_KEYS = ("length", "n_sequences", "gap_fraction", "conservation", "identity")


def _rows(aln):
    """one alignment as the reference takes it: a non-empty list of str of one length -> bytes rows (latin-1)"""
    aln = list(aln)
    if not aln:
        raise ValueError("Empty alignment provided")
    rows = [x.encode("latin-1") if isinstance(x, str) else bytes(x) for x in aln]
    if len(set(len(r) for r in rows)) > 1:
        raise ValueError("All sequences in alignment must have the same length")
    return rows


def _families(families):
    families = list(families)
    if not families:
        raise ValueError("Empty list of alignments provided")
    return [_rows(f) for f in families]


def _threshold(t, n=None):
    """one threshold, or one per family, each in [0, 1] as the reference asks"""
    many = n is not None and hasattr(t, "__len__")
    ts = [float(x) for x in t] if many else [float(t)]
    if many and len(ts) != n:
        raise ValueError("%d thresholds for %d alignments" % (len(ts), n))
    for x in ts:
        if not 0 <= x <= 1:
            raise ValueError("Threshold must be between 0 and 1")
    return ts if many else ts[0]


def _summary(ctx, fams):
    if any(len(f[0]) == 0 for f in fams):
        raise KalignAmdError("an alignment of width 0 has no summary")
    return ctx.family_summary(fams, gap=b"-")


def alignment_stats_families(ctx, families):
    """alignment_stats of every alignment of the list: dicts with the reference's keys"""
    s = _summary(ctx, _families(families))
    try:
        return [{k: d[k] for k in _KEYS} for d in s.summary()]
    finally:
        s.close()


def consensus_sequences(ctx, families, threshold=0.5):
    """consensus_sequence of every alignment of the list (threshold: one value or one per alignment): a list of str"""
    fams = _families(families)
    t = _threshold(threshold, len(fams))
    s = _summary(ctx, fams)
    try:
        return [c.decode("latin-1") for c in s.consensus(t)]
    finally:
        s.close()


def remove_gap_columns_families(ctx, families, threshold=1.0):
    """remove_gap_columns of every alignment of the list (threshold: one value or one per alignment): lists of str"""
    fams = _families(families)
    t = _threshold(threshold, len(fams))
    s = _summary(ctx, fams)
    try:
        return [[r.decode("latin-1") for r in f] for f in s.compact(gap_threshold=t)]
    finally:
        s.close()


def pairwise_identity_matrices(ctx, families):
    """pairwise_identity_matrix of every alignment of the list: float64 [n, n] arrays, all from one launch"""
    s = _summary(ctx, _families(families))
    try:
        return s.identity()
    finally:
        s.close()


def gap_stats_families(ctx, families):
    """compute_gap_stats of the reference's benchmarks/analysis.py for every alignment of the list (rows as str or bytes):
    dicts with GapStats' field names, and with gap_opens_per_seq, characters, terminal_gaps and internal_gaps"""
    s = _summary(ctx, _families(families))
    try:
        return s.gaps()
    finally:
        s.close()


def dealign_families(ctx, families):
    """every alignment of the list without its gaps (the reference's dealign_msa): per alignment the list of its sequences,
    str where its rows were str and bytes where they were bytes; a row of gaps alone gives an empty sequence"""
    families = [list(f) for f in families]
    text = [bool(f) and isinstance(f[0], str) for f in families]
    s = _summary(ctx, _families(families))
    try:
        out = s.ungapped()
    finally:
        s.close()
    return [[r.decode("latin-1") for r in rows] if t else rows for rows, t in zip(out, text)]


def gap_stats(ctx, alignment):
    """benchmarks/analysis.py: compute_gap_stats of one alignment: expansion factor, gap blocks and their mean length,
    terminal against internal gaps per sequence, gappy columns"""
    return gap_stats_families(ctx, [alignment])[0]


def dealign(ctx, alignment):
    """one alignment's sequences without their gaps, in the type they were given"""
    return dealign_families(ctx, [alignment])[0]


def alignment_stats(ctx, alignment):
    """kalign.utils.alignment_stats: length, n_sequences, gap_fraction, conservation, identity"""
    return alignment_stats_families(ctx, [alignment])[0]


def consensus_sequence(ctx, alignment, threshold=0.5):
    """kalign.utils.consensus_sequence: 'N' (nucleotides) or 'X' where no character reaches the threshold"""
    return consensus_sequences(ctx, [alignment], _threshold(threshold))[0]


def remove_gap_columns(ctx, alignment, threshold=1.0):
    """kalign.utils.remove_gap_columns: the columns whose gap fraction is below the threshold"""
    return remove_gap_columns_families(ctx, [alignment], _threshold(threshold))[0]


def pairwise_identity_matrix(ctx, alignment):
    """kalign.utils.pairwise_identity_matrix: the symmetric [n, n] matrix of identities over the columns where both
    sequences hold a character; 1.0 on the diagonal, 0.0 for a pair that shares no column"""
    return pairwise_identity_matrices(ctx, [alignment])[0]


def trim_range(length, start=None, end=None):
    """trim_alignment's range rules: None is the alignment's end, a negative index counts from the right (not below 0),
    start >= end is refused.  Returns (start, end) as a slice takes them."""
    def place(x, missing):
        return missing if x is None else x if x >= 0 else max(0, length + x)

    lo, hi = place(start, 0), place(end, length)
    if not lo < hi:
        raise ValueError("Start position must be less than end position")
    return lo, hi


def trim_alignment(ctx, alignment, start=None, end=None):
    """kalign.utils.trim_alignment: the columns start (inclusive) to end (exclusive), the range handed to the device as a
    column mask"""
    rows = _rows(alignment)
    w = len(rows[0])
    start, end = trim_range(w, start, end)
    mask = [1 if start <= c < end else 0 for c in range(w)]
    s = _summary(ctx, [rows])
    try:
        return [r.decode("latin-1") for r in s.compact(column_masks=[mask])[0]]
    finally:
        s.close()


def mask_by_confidence(ctx, families, column_confidences, threshold):
    """mask_alignment_by_confidence of the reference's benchmarks/downstream/utils.py for a list of alignments: column j of
    family f is kept when float(column_confidences[f][j]) >= threshold, compared in double as the reference compares
    them.  The flags go to the device as column masks (FamilySummary.compact).  Returns (rows, n_retained) per family."""
    fams = _families(families)
    conf = list(column_confidences)
    if len(conf) != len(fams):
        raise ValueError("%d confidence lists for %d alignments" % (len(conf), len(fams)))
    t = float(threshold)
    masks = []
    for f, (rows, c) in enumerate(zip(fams, conf)):
        if len(c) != len(rows[0]):
            raise ValueError("alignment %d: %d confidences for %d columns" % (f, len(c), len(rows[0])))
        masks.append([1 if float(x) >= t else 0 for x in c])
    s = _summary(ctx, fams)
    try:
        out = s.compact(column_masks=masks)
    finally:
        s.close()
    return [([r.decode("latin-1") for r in rows], len(rows[0]) if rows else 0) for rows in out]
