"""Records tests/golden/cod_*.npz: inputs of the codon stage and what the reference makes of them.  Needs the reference's
sources (its benchmarks/downstream/positive_selection.py, loaded as a module: it imports nothing outside the standard
library) and the compiled reference (make -C oracle ref); run from the repository root:
    python tests/golden/make_codon_golden.py <path of the reference>

A text field NAME is uint8, the strings one after the other, with NAME_off (int64 [n + 1]) beside it.
  cod_table            codons: the 64 codons in A C G T order; aa: what _translate_dna makes of each ("" for a stop)
  cod_translate_*      dna: sequences; protein: _translate_dna of each
  cod_back_*           dna: sequences; rows: a hand-gapped protein row for each; codon_rows: _backtranslate(row, dna)
  cod_e2e_*            dna and fam_first (int32 [n_fam + 1]): coding sequences of a few families; protein: _translate_dna of
                       each; protein_rows: the reference's alignment of each family's proteins (oracle.refdrv.RefJob,
                       run_tree() + finalise(), rows in input order); codon_rows: _backtranslate of those; n_anchors, weight,
                       subm [529] and scal [6] as the reference chose them (the same for every family)
Data only: no program text of the reference is stored."""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import refdrv  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
PROT = "ACDEFGHIKLMNPQRSTVWY"
STOPS = ("TAA", "TAG", "TGA")


def reference(path):
    spec = importlib.util.spec_from_file_location("positive_selection", os.path.join(path, "benchmarks", "downstream", "positive_selection.py"))
    m = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = m           # (its dataclasses look their module up)
    spec.loader.exec_module(m)
    return m


def pack(strs):
    bs = [s.encode("latin-1") if isinstance(s, str) else s for s in strs]
    off = np.zeros(len(bs) + 1, np.int64)
    off[1:] = np.cumsum([len(b) for b in bs])
    return np.frombuffer(b"".join(bs), np.uint8).copy(), off


def save(name, texts, **kw):
    d = dict(kw)
    for k, v in texts.items():
        d[k], d[k + "_off"] = pack(v)
    np.savez_compressed(os.path.join(OUT, "cod_%s.npz" % name), **d)
    print("cod_%s: %s" % (name, {k: len(v) for k, v in texts.items()}))


def protein_family(rng, n, lo, hi, p_sub=0.2, p_indel=0.05):
    """n descendants of one random root protein, lengths roughly lo .. hi"""
    a = np.frombuffer(PROT.encode(), np.uint8)
    root = rng.choice(a, size=int(rng.integers(lo, hi + 1)))
    out = []
    for _ in range(n):
        s = []
        for c in root:
            r = rng.random()
            if r < p_indel:
                continue
            s.append(int(rng.choice(a)) if r < p_indel + p_sub else int(c))
            if rng.random() < p_indel:
                s.append(int(rng.choice(a)))
        out.append(bytes(s[:hi]).decode())
    return out


def thread(rng, protein, codons_of, p_stop=0.02):
    """a coding sequence of the protein: a random codon per amino acid, a few in-frame stops, one at the end"""
    out = []
    for aa in protein:
        if rng.random() < p_stop:
            out.append(STOPS[int(rng.integers(0, 3))])
        out.append(codons_of[aa][int(rng.integers(0, len(codons_of[aa])))])
    out.append(STOPS[int(rng.integers(0, 3))])
    return "".join(out)


def gapped(rng, protein, width, lead=0, trail=0):
    """the protein spread over `width` columns: `lead` gaps first, `trail` last, the rest in runs"""
    free = width - len(protein) - lead - trail
    assert free >= 0
    cuts = sorted(int(x) for x in rng.integers(0, len(protein) + 1, size=3))
    runs = [free // 3, free // 3, free - 2 * (free // 3)]
    row, k = "-" * lead, 0
    for cut, run in zip(cuts, runs):
        row += protein[k:cut] + "-" * run
        k = cut
    return row + protein[k:] + "-" * trail


def main():
    ref = reference(sys.argv[1])
    tr, back = ref._translate_dna, ref._backtranslate
    rng = np.random.default_rng(20261021)
    codons = [a + b + c for a in "ACGT" for b in "ACGT" for c in "ACGT"]
    aa = [tr(c) for c in codons]
    save("table", dict(codons=codons, aa=aa))
    codons_of = {}
    for c, x in zip(codons, aa):
        if x:
            codons_of.setdefault(x, []).append(c)
    assert sorted(codons_of) == sorted(PROT) and sum(1 for x in aa if not x) == 3

    def translate_case(name, dna):
        save("translate_" + name, dict(dna=dna, protein=[tr(s) for s in dna]))

    every = "".join(codons)
    translate_case("all64", [every, every[::-1], "".join(codons[int(k)] for k in rng.permutation(64))] + codons)
    translate_case("case", [every.lower(), "".join(c if k % 2 else c.lower() for k, c in enumerate(every)), "atgGCCtaaTtT", "AtGgCcTaAtTt"])
    others = "NURYSWKMBDHVXEFIJLOPQZ"
    translate_case("other_letters", [x + "CG" for x in others] + ["A" + x + "G" for x in others] + ["AC" + x for x in others] +
                   [x.lower() + "cg" for x in others] + ["ATGNNNGCC", "UUUUAAUAG", "ATGGCNTAATGN", "NNN", "TAN", "TNA", "NAA", "UAA", "UGA", "TRA"])
    translate_case("stops", ["TAAATGGCC", "ATGGCCTGA", "ATGTAATAGTGAGCC", "TAATAGTGATAAATG", "ATGTAATAGTGATAA", "TAGTGAGCCTAATAA",
                             "taaATGtagGCCtga", "TAA" * 70 + "ATG", "ATG" + "TGA" * 70, "TAG" * 31 + "GCC" + "TAG" * 40])

    # ---- backtranslate: hand-gapped rows, gaps leading, trailing and in runs ----
    dna, rows = [], []
    for n_aa, width, lead, trail in ((1, 1, 0, 0), (1, 5, 4, 0), (1, 5, 0, 4), (7, 20, 3, 5), (20, 20, 0, 0), (30, 64, 10, 0), (40, 65, 0, 12),
                                     (63, 130, 30, 30), (100, 257, 1, 1), (120, 300, 100, 60)):
        p = "".join(rng.choice(list(PROT), size=n_aa))
        s = thread(rng, p, codons_of, p_stop=0.1)
        s = s.lower() if len(dna) % 3 == 1 else s
        assert tr(s) == p
        dna.append(s)
        rows.append(gapped(rng, p, width, lead, trail))
    dna.append("ATGNNNuuuTAAGCC")
    rows.append("-MX--XA-")
    save("back_rows", dict(dna=dna, rows=rows, codon_rows=[back(r, s) for r, s in zip(rows, dna)]))

    # ---- end to end: four families, in the reference's fast and default mode ----
    fams = []
    for n, lo, hi in ((2, 34, 40), (5, 60, 90), (16, 100, 140), (9, 150, 185)):
        fam = [thread(rng, p, codons_of) for p in protein_family(rng, n, lo, hi)]
        fam[1] = fam[1].lower()
        assert all(90 <= len(s) <= 600 for s in fam)
        fams.append(fam)
    first = np.zeros(len(fams) + 1, np.int32)
    first[1:] = np.cumsum([len(f) for f in fams])
    for name, n_anchors in (("e2e_fast", 0), ("e2e_default", 5)):
        prot, prows, crows, subm, scal = [], [], [], [], []
        for fam in fams:
            p = [tr(s) for s in fam]
            job = refdrv.RefJob(p)
            assert job.biotype == 0, "the reference no longer calls the translated family protein"
            if n_anchors:
                job.build_consistency(n_anchors, 2.0)
            job.run_tree()
            r = job.finalise()
            assert [x.replace("-", "") for x in r] == p, "rows in input order"
            prot += p
            prows += r
            crows += [back(x, s) for x, s in zip(r, fam)]
            subm.append(job.subm.copy())
            scal.append(np.array([job.gpo, job.gpe, job.tgpe, job.dist_scale, job.vsm_amax, job.use_seq_weights], np.float32))
        assert all(np.array_equal(subm[0], x) for x in subm) and all(np.array_equal(scal[0], x) for x in scal)
        save(name, dict(dna=[s for f in fams for s in f], protein=prot, protein_rows=prows, codon_rows=crows), fam_first=first,
             n_anchors=np.int32(n_anchors), weight=np.float32(2.0), subm=subm[0], scal=scal[0])


if __name__ == "__main__":
    main()
