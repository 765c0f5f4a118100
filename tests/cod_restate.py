"""A numpy restatement of the codon stage (include/kalign_amd.h, the codon stage): residues by the input stage's byte rule,
upper-cased; three residues a codon; the standard code over exactly A C G T, X for any other letter; stop codons omitted;
a protein row's gap byte three gap bytes, its k-th residue the k-th non-stop codon -- written from the rule's text, sharing
nothing with the library.  tests/test_codon_host.py holds it to the goldens recorded from the reference
(tests/golden/cod_*.npz), tests/test_gpu_codon.py holds the library to it."""
import glob
import os

import numpy as np

import in_restate as ir

SEQ = ("residues", "gap_characters", "dropped", "codons", "stops", "x_codons")
# the standard code written out by amino acid (NCBI table 1), not as the library's 64-letter string
CODE = {"F": "TTT TTC", "L": "TTA TTG CTT CTC CTA CTG", "I": "ATT ATC ATA", "M": "ATG", "V": "GTT GTC GTA GTG",
        "S": "TCT TCC TCA TCG AGT AGC", "P": "CCT CCC CCA CCG", "T": "ACT ACC ACA ACG", "A": "GCT GCC GCA GCG", "Y": "TAT TAC",
        "*": "TAA TAG TGA", "H": "CAT CAC", "Q": "CAA CAG", "N": "AAT AAC", "K": "AAA AAG", "D": "GAT GAC", "E": "GAA GAG",
        "C": "TGT TGC", "W": "TGG", "R": "CGT CGC CGA CGG AGA AGG", "G": "GGT GGC GGA GGG"}
AA = {c: aa for aa, cs in CODE.items() for c in cs.split()}
assert len(AA) == 64
CODONS = [a + b + c for a in "ACGT" for b in "ACGT" for c in "ACGT"]


def table():
    """the 64 letters in the order 16a + 4b + c with A 0, C 1, G 2, T 3"""
    return "".join(AA[c] for c in CODONS).encode()


def residues(s):
    """the sequence's letters, upper-cased, as a str, and its counts of residues, gap characters and dropped bytes; raises
    as the stage refuses a byte >= 128"""
    b = ir.raw(s)
    let, pun, high = ir.is_letter(b), ir.is_punct(b), b >= 128
    if high.any():
        raise ValueError("byte 0x%02x at offset %d" % (b[np.argmax(high)], np.argmax(high)))
    return b[let].tobytes().decode().upper(), dict(residues=int(let.sum()), gap_characters=int(pun.sum()), dropped=int((~let & ~pun).sum()))


def translate(s):
    """one sequence -> dict: protein (str), kept (the DNA without stop codons, upper-cased, str) and rec (the six counts of
    SEQ); raises ValueError as the stage refuses"""
    dna, r = residues(s)
    if len(dna) % 3:
        raise ValueError("%d residues, not a multiple of 3" % len(dna))
    codons = [dna[k:k + 3] for k in range(0, len(dna), 3)]
    aas = [AA.get(c, "X") for c in codons]
    keep = [c for c, a in zip(codons, aas) if a != "*"]
    if not keep:
        raise ValueError("no protein")
    return dict(protein="".join(a for a in aas if a != "*"), kept="".join(keep),
                rec=[r["residues"], r["gap_characters"], r["dropped"], len(codons), aas.count("*"), aas.count("X")])


def backtranslate(row, s, gap="-"):
    """a protein row (str / bytes) over the coding sequence s -> the codon row (str); raises ValueError on a count mismatch"""
    row = row.decode("latin-1") if isinstance(row, (bytes, bytearray)) else row
    kept = translate(s)["kept"]
    n = sum(ch != gap for ch in row)
    if 3 * n != len(kept):
        raise ValueError("the row holds %d residues, the sequence %d codons without stops" % (n, len(kept) // 3))
    out, k = [], 0
    for ch in row:
        if ch == gap:
            out.append(gap * 3)
        else:
            out.append(kept[3 * k:3 * k + 3])
            k += 1
    return "".join(out)


class CodGolden:
    """one tests/golden/cod_*.npz (see tests/golden/make_codon_golden.py for the fields): lists of bytes for every packed
    text (NAME / NAME_off), arrays for the rest"""

    def __init__(self, path):
        z = np.load(path)
        self.name = os.path.basename(path)[4:-4]
        self.z = {k: z[k] for k in z.files}

    def has(self, k):
        return k in self.z

    def texts(self, k):
        t, o = self.z[k], self.z[k + "_off"]
        return [t[o[i]:o[i + 1]].tobytes() for i in range(len(o) - 1)]

    def families(self, k):
        """a packed text dealt to the golden's families (fam_first)"""
        t, first = self.texts(k), self.z["fam_first"]
        return [t[first[f]:first[f + 1]] for f in range(len(first) - 1)]

    def __getattr__(self, k):
        try:
            return self.__dict__["z"][k]
        except KeyError:
            raise AttributeError(k)


def goldens(golden_dir):
    return {g.name: g for g in (CodGolden(p) for p in sorted(glob.glob(os.path.join(golden_dir, "cod_*.npz"))))}
