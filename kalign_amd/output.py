"""From rows to alignment text: the output stage (Context.family_output = ka_out_fam) for a batch of families.

The reference writes an alignment one row and one line at a time (lib/src/msa_io.c: write_msa_fasta, write_msa_clu,
write_msa_msf; python-kalign/io.py: write_fasta, write_stockholm).  Here the rows and names of every family go to the device
once, and each format is written for the whole batch by one launch into one buffer that comes back in one piece -- the same
bytes the reference writes.  The ensemble's residue_confidence / column_confidence become Stockholm PP lines
(stockholm_families).  There is no CPU fallback: every function takes a Context."""
import os

from .api import CLUSTAL_HEADER, MSF_DATE, OUT_STATS, KalignAmdError, pp_char  # noqa: F401

FORMATS = ("fasta", "clustal", "msf", "stockholm")


def _names(names):
    return None if names is None else [list(n) for n in names]


def format_families(ctx, families_rows, names, fmt, gap=b"-", **kw):
    """one text (bytes) per family.  fmt and its keywords:
      "fasta"      line_length=60 (write_msa_fasta; 80 is kalign.io.write_fasta's default)
      "clustal"    header=CLUSTAL_HEADER
      "msf"        titles (one per family), biotypes (0 protein / 1 DNA, one value or one per family), date=None (now)
      "stockholm"  residue_confidence and / or column_confidence, one array per family
    names: a list of lists like families_rows, or None (seq0, seq1, ... per family)."""
    if fmt not in FORMATS:
        raise KalignAmdError("format %r is not one of %s" % (fmt, ", ".join(FORMATS)))
    out = ctx.family_output(families_rows, names=_names(names), gap=gap)
    try:
        return getattr(out, fmt)(**kw)
    finally:
        out.close()


def format_alignment(ctx, rows, names, fmt, gap=b"-", **kw):
    """one family: a batch of one.  The per-family keywords of format_families take the family's own value: title, biotype,
    residue_confidence [n, W], column_confidence [W]."""
    if "title" in kw:
        kw["titles"] = [kw.pop("title")]
    if "biotype" in kw:
        kw["biotypes"] = [kw.pop("biotype")]
    for k in ("residue_confidence", "column_confidence"):
        if kw.get(k) is not None:
            kw[k] = [kw[k]]
    return format_families(ctx, [list(rows)], None if names is None else [list(names)], fmt, gap=gap, **kw)[0]


def write_families(ctx, families_rows, names, fmt, paths, gap=b"-", **kw):
    """format_families, one file per family; the MSF title of a family is its path's basename, as the reference's is.  Returns
    the texts."""
    paths = [os.fspath(p) for p in paths]
    if len(paths) != len(families_rows):
        raise KalignAmdError("%d paths for %d families" % (len(paths), len(families_rows)))
    if fmt == "msf" and "titles" not in kw:
        kw["titles"] = [os.path.basename(p) for p in paths]
    texts = format_families(ctx, families_rows, names, fmt, gap=gap, **kw)
    for p, t in zip(paths, texts):
        with open(p, "wb") as f:
            f.write(t)
    return texts


def stockholm_families(ctx, results, names=None, gap=b"-"):
    """the Stockholm text with PP lines of every family of an ensemble: results are the dicts ensemble.finish_ensembles returns
    (rows, residue_confidence, column_confidence)."""
    return format_families(ctx, [r["rows"] for r in results], names, "stockholm", gap=gap,
                           residue_confidence=[r["residue_confidence"] for r in results],
                           column_confidence=[r["column_confidence"] for r in results])
