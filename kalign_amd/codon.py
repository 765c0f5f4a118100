"""Coding DNA aligned in frame: translate, align the proteins, backtranslate -- the codon stage (Context.family_codons =
ka_cod_fam) for a batch of families.

A nucleotide alignment of coding sequences puts one- and two-base gaps where they score well, which breaks the reading
frame for every codon model downstream.  Here a sequence's letters (the input stage's byte rule, upper-cased) are read three
a codon, translated with the standard code over exactly A C G T (any other letter makes the codon X; U is not T), stop codons
omitted wherever they stand; the proteins are aligned as protein families with the caller's (subm, scal); and every protein
column becomes three nucleotide columns.  What the reference's positive-selection pipeline does one family at a time on the
host (benchmarks/downstream/positive_selection.py: _translate_dna, _backtranslate).  There is no CPU fallback: every
function takes a Context."""
import numpy as np

from . import summary
from .api import COD_SEQ, KalignAmdError  # noqa: F401


def _names(names):
    return None if names is None else [list(n) for n in names]


def translate_families(ctx, families, names=None):
    """per family (proteins, records): the proteins (bytes) in input order and an int32 array [n, 6] of residues, gap
    characters, dropped bytes, codons, stop codons and X codons (COD_SEQ)"""
    cod = ctx.family_codons(families, names=_names(names))
    try:
        return list(zip(cod.proteins(), cod.sequences()))
    finally:
        cod.close()


def align_codon_families(ctx, families, subm, scal, names=None, n_anchors=0, weight=2.0, realign=0, refine=0, n_threads=4, gap=b"-",
                         want_protein=False):
    """families: a list of lists of coding sequences.  subm, scal: the protein's parameters.  Returns one list of codon rows
    (bytes) per family, in the caller's order, each of width three times its protein alignment's; want_protein: also the
    protein rows, second."""
    cod = ctx.family_codons(families, names=_names(names))
    try:
        cod.run(subm, scal, n_anchors=n_anchors, weight=weight, realign=realign, refine=refine, n_threads=n_threads, gap=gap)
        rows = cod.rows()
        return (rows, cod.protein_rows()) if want_protein else rows
    finally:
        cod.close()


def align_codons(ctx, seqs, subm, scal, names=None, want_protein=False, **kw):
    """one family: a batch of one.  Returns its codon rows (bytes) in the order of seqs (want_protein: and its protein rows)."""
    out = align_codon_families(ctx, [list(seqs)], subm, scal, names=None if names is None else [list(names)], want_protein=want_protein, **kw)
    return (out[0][0], out[1][0]) if want_protein else out[0]


def backtranslate_families(ctx, families, protein_rows, gap=b"-"):
    """the codon rows of protein rows the caller brings -- one list of rows per family, rows in the order of the sequences --
    over the coding sequences in families.  A row whose residues are not as many as its sequence's non-stop codons is
    refused."""
    cod = ctx.family_codons(families)
    try:
        cod.back([[r.encode("latin-1") if isinstance(r, str) else bytes(r) for r in f] for f in protein_rows], gap=gap)
        return cod.rows()
    finally:
        cod.close()


def mask_by_confidence(ctx, codon_families, protein_column_confidences, threshold):
    """confidence masking at the codon level (the reference's positive_selection.py:499-507): each protein column's
    confidence stands for its three nucleotide columns, then summary.mask_by_confidence as it stands.  Returns (rows,
    n_retained) per family."""
    return summary.mask_by_confidence(ctx, codon_families, [np.repeat(np.asarray(c, np.float64), 3) for c in protein_column_confidences],
                                      threshold)
