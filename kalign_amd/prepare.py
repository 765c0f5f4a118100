"""From sequences as a user has them to rows in the user's order: the input stage (Context.family_input = ka_in_fam) in
front of the batch of families.

A sequence is a str or bytes: letters are residues (case is kept, ambiguity codes included), punctuation is gap characters
-- an already aligned input is dealigned, as the reference does -- and white space and digits are dropped.  Per family the
stage detects protein or nucleotides, sorts by length and name as the reference sorts, encodes in the guide tree's and the
alignment's alphabets, aligns, and puts the rows back in the order they were given in.  Substitution matrices are the
caller's (subm, scal), as everywhere in this package.  There is no CPU fallback: every function takes a Context."""
import numpy as np

from .api import IN_FAM, IN_SEQ, KalignAmdError  # noqa: F401

PROTEIN, DNA = 0, 1
ALIGNED_STATUS = {1: "unaligned", 2: "aligned", 3: "unknown"}


def pfasum_auto(min_len, max_len):
    """the matrix the reference's auto type picks for a protein family (resolve_pfasum_auto): PFASUM43 when the float32
    ratio of the longest to the shortest sequence is below 1.5 (or the shortest is empty), else PFASUM60; as a str"""
    ratio = np.float32(max_len) / np.float32(min_len) if min_len > 0 else np.float32(1.0)
    return "PFASUM43" if ratio < np.float32(1.5) else "PFASUM60"


def prepare_families(ctx, families, names=None, biotype=None, want_input=False):
    """per family a dict: biotype, status (1 unaligned, 2 aligned, 3 unknown), min_len, max_len, no_code, lens / gap_characters
    / dropped / checksums (input order), order (sorted position -> input index) and the three encodings tree_codes, codes,
    letters (sorted order, as Context.run_families takes them).  want_input: also the FamilyInput itself, second."""
    inp = ctx.family_input(families, names=names, biotype=biotype)
    out = []
    for fam, seqs, order, enc in zip(inp.families(), inp.sequences(), inp.order(), inp.encoded()):
        d = dict(biotype=fam["biotype"], status=fam["aligned"], min_len=fam["min_len"], max_len=fam["max_len"], no_code=fam["no_code"],
                 lens=seqs[:, 0].copy(), gap_characters=seqs[:, 1].copy(), dropped=seqs[:, 2].copy(), checksums=seqs[:, 3].copy(),
                 order=order, tree_codes=enc[0], codes=enc[1], letters=enc[2])
        out.append(d)
    if want_input:
        return out, inp
    inp.close()
    return out


def _params(params, biotypes):
    """{biotype: (subm, scal)} for the biotypes of the batch"""
    if isinstance(params, dict):
        missing = sorted(set(biotypes) - set(params))
        if missing:
            raise KalignAmdError("align_families: no parameters for biotype %d" % missing[0])
        return {b: params[b] for b in sorted(set(biotypes))}
    if len(set(biotypes)) > 1:
        raise KalignAmdError("align_families: protein and nucleotide families in one batch need parameters per biotype: "
                             "{0: (subm, scal), 1: (subm, scal)}")
    return {biotypes[0]: params}


def align_families(ctx, families, params, names=None, biotype=None, n_anchors=0, weight=2.0, realign=0, refine=0, n_threads=4,
                   gap=b"-", want_input=False):
    """families: a list of lists of sequences.  params: one (subm, scal) -- then all families share a biotype -- or
    {0: (subm, scal), 1: (subm, scal)}.  Returns one list of rows (bytes) per family, in the caller's order; want_input:
    also the FamilyInput (its families(), sequences(), stats()), second."""
    inp = ctx.family_input(families, names=names, biotype=biotype)
    try:
        for b, (subm, scal) in _params(params, [f["biotype"] for f in inp.families()]).items():
            inp.run(b, subm, scal, n_anchors=n_anchors, weight=weight, realign=realign, refine=refine, n_threads=n_threads, gap=gap)
        rows = inp.rows()
    except Exception:
        inp.close()
        raise
    if want_input:
        return rows, inp
    inp.close()
    return rows


def align(ctx, seqs, subm, scal, names=None, biotype=None, **kw):
    """one family: a batch of one.  Returns its rows (bytes) in the order of seqs."""
    return align_families(ctx, [list(seqs)], (subm, scal), names=None if names is None else [list(names)], biotype=biotype, **kw)[0]
