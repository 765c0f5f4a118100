"""Records tests/golden/in_*.npz: inputs of the input stage and what the reference makes of them.  Needs the compiled
reference (make -C oracle ref cli); run from the repository root:  python tests/golden/make_input_golden.py

Every file holds the input -- text (uint8, the sequences' raw bytes one after the other), seq_off (int64 [n + 1]), and
names / name_off the same way where the case has names -- and recorded results:
  letter-only inputs, through oracle.refdrv.RefJob (the reference's library entry: names "s%07d"):
    biotype, lens and ranks (sorted position -> input index), tree_codes and codes (flat, sorted order)
  end-to-end cases: rows (uint8 [n, alnlen], INPUT order), subm, scal, n_anchors, weight -- RefJob.run_tree() + finalise()
    for letter-only inputs; for FASTA files (route = "cli") the output of the reference's CLI with the parameters in
    force (refdrv.param_table)
  status cases: status, written down by hand from detect_aligned's four branches (the library entry does not hand the
    reference's value out)
Data only: no program text of the reference is stored."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import refdrv  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
CLI = os.path.join(ROOT, "oracle", "_ref", "kalign_ref")
PROT = "ACDEFGHIKLMNPQRSTVWY"
NUC = "ACGT"
UPPER = "".join(chr(c) for c in range(65, 91))
LOWER = UPPER.lower()


def pack(strs):
    bs = [s.encode("latin-1") if isinstance(s, str) else s for s in strs]
    off = np.zeros(len(bs) + 1, np.int64)
    off[1:] = np.cumsum([len(b) for b in bs])
    return np.frombuffer(b"".join(bs), np.uint8).copy(), off


def save(name, seqs, names=None, **kw):
    text, off = pack(seqs)
    d = dict(text=text, seq_off=off)
    if names is not None:
        d["names"], d["name_off"] = pack(names)
    d.update(kw)
    np.savez_compressed(os.path.join(OUT, "in_%s.npz" % name), **d)
    print("in_%s: %d sequences, %s" % (name, len(seqs), sorted(kw)))


def family(rng, alphabet, n, lo, hi, p_sub=0.2, p_indel=0.05):
    """n descendants of one random root, lengths roughly lo .. hi"""
    a = np.frombuffer(alphabet.encode(), np.uint8)
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


def ref_fields(job):
    return dict(biotype=np.int32(job.biotype), lens=job.lens.copy(), ranks=job.ranks.copy(),
                tree_codes=np.concatenate(job.tree_codes), codes=np.concatenate(job.codes))


def ref_rows(job, n_anchors, weight=2.0):
    if n_anchors:
        job.build_consistency(n_anchors, weight)
    job.run_tree()
    rows = job.finalise()
    return np.array([np.frombuffer(r.encode(), np.uint8) for r in rows])


def cli_rows(seqs, names, flags):
    """the reference's CLI on a FASTA file with these sequence lines (one line per sequence, no blanks): rows in input order"""
    with tempfile.TemporaryDirectory() as tmp:
        inp, out = os.path.join(tmp, "in.fa"), os.path.join(tmp, "out.fa")
        with open(inp, "w") as f:
            for n, s in zip(names, seqs):
                f.write(">%s\n%s\n" % (n, s))
        subprocess.run([CLI, "-i", inp, "-o", out, "-f", "fasta", "-n", "1"] + flags, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        got, rows = [], []
        for line in open(out):
            line = line.rstrip("\n")
            if line.startswith(">"):
                got.append(line[1:])
                rows.append("")
            else:
                rows[-1] += line
    assert got == list(names), (got, names)
    assert len(set(len(r) for r in rows)) == 1
    return np.array([np.frombuffer(r.encode(), np.uint8) for r in rows])


def strip(s):
    return "".join(c for c in s if c.isalpha())


def main():
    rng = np.random.default_rng(20261021)

    # ---- the full tables ----
    fam = family(rng, PROT, 6, 50, 70)
    fam[2] = fam[2][:20] + UPPER + fam[2][20:30] + LOWER + fam[2][30:]
    fam[4] = fam[4].lower()
    job = refdrv.RefJob(fam)
    assert job.biotype == 0, "the reference no longer calls the full protein family protein"
    save("table_protein", fam, **ref_fields(job))
    fam = family(rng, NUC, 6, 90, 120)
    fam[1] = fam[1][:30] + UPPER + fam[1][30:50] + LOWER + fam[1][50:]
    fam[3] = fam[3].lower()
    job = refdrv.RefJob(fam)
    assert job.biotype == 1, "the reference no longer calls the full nucleotide family DNA"
    save("table_dna", fam, **ref_fields(job))

    # ---- the detection edge: eight and nine letters of ACGTUN per other protein letter; what the reference says is recorded ----
    for k, unit in ((8, "ACGTACGTK"), (9, "ACGTACGTAK")):
        fam = [unit * m for m in (5, 3, 4)]
        job = refdrv.RefJob(fam)
        save("edge%d" % k, fam, **ref_fields(job))
        print("   edge%d: biotype %d" % (k, job.biotype))

    # ---- equal lengths ----
    fam = family(rng, PROT, 7, 40, 40, p_indel=0.0)
    assert len(set(len(s) for s in fam)) == 1
    job = refdrv.RefJob(fam)
    save("equal_unnamed", fam, n_anchors=np.int32(0), weight=np.float32(2.0), subm=job.subm.copy(),
         scal=np.array([job.gpo, job.gpe, job.tgpe, job.dist_scale, job.vsm_amax, job.use_seq_weights], np.float32), **ref_fields(job),
         rows=ref_rows(job, 0))
    names = ["seq_d", "seq_b", "seq_g", "seq_a", "seq_c", "seq_f", "seq_e"]
    subm, scal = refdrv.param_table(0, 5)
    save("equal_named", fam, names=names, route="cli", biotype=np.int32(0), n_anchors=np.int32(0), weight=np.float32(2.0), subm=subm.reshape(-1), scal=scal,
         rows=cli_rows(fam, names, ["--fast", "--type", "pfasum43"]))

    # ---- one family per aligned status (detect_aligned's four branches) ----
    save("status_unaligned", ["ACDEFGHIK", "ACDEFGH", "ACDEF"], status=np.int32(1))          # no gap character, lengths differ
    save("status_aligned", ["ACD-EFG.HIK", "A-DEEFGHH-K", "--DEEFGH..K"], status=np.int32(2))   # gap characters, one total length
    save("status_unknown_gaps", ["ACD-EFGHIK", "ACDEFG-H", "ACDEF"], status=np.int32(3))        # gap characters, totals differ
    save("status_unknown_same", ["ACDEFGHIK", "ACDEFGHIR", "ACDKFGHIK"], status=np.int32(3))    # no gap character, one length

    # ---- end to end: per biotype a fast-mode and a default-mode case ----
    for name, alphabet, n, lo, hi, n_anchors in (("e2e_protein_fast", PROT, 12, 60, 100, 0), ("e2e_protein_default", PROT, 10, 60, 100, 5),
                                                 ("e2e_dna_fast", NUC, 12, 70, 110, 0), ("e2e_dna_default", NUC, 9, 70, 110, 5)):
        fam = family(rng, alphabet, n, lo, hi)
        job = refdrv.RefJob(fam)
        assert job.biotype == (0 if alphabet == PROT else 1)
        save(name, fam, n_anchors=np.int32(n_anchors), weight=np.float32(2.0), subm=job.subm.copy(),
             scal=np.array([job.gpo, job.gpe, job.tgpe, job.dist_scale, job.vsm_amax, job.use_seq_weights], np.float32), **ref_fields(job),
             rows=ref_rows(job, n_anchors))

    # ---- the file route: an already aligned, mixed-case FASTA input with '-' and '.', default mode, through the CLI ----
    base = [s[:45 + 3 * k] for k, s in enumerate(family(rng, NUC, 8, 60, 90))]
    assert len(set(len(s) for s in base)) == len(base), "distinct lengths: the order does not depend on the names"
    width = max(len(s) for s in base) + 6
    fam = []
    for k, s in enumerate(base):
        s = s.lower() if k % 3 == 1 else s
        row = list(s)
        while len(row) < width:
            row.insert(int(rng.integers(0, len(row) + 1)), "-" if rng.random() < 0.6 else ".")
        fam.append("".join(row))
    names = ["n%02d some description" % k for k in range(len(fam))]
    subm, scal = refdrv.param_table(1, 0)
    rows = cli_rows(fam, names, ["--type", "dna"])
    # the same letters through the library entry give the same rows: the CLI's parameters are the ones recorded
    job = refdrv.RefJob([strip(s) for s in fam], type_=0)
    assert job.biotype == 1 and np.array_equal(job.subm, subm.reshape(-1))
    assert np.array_equal(ref_rows(job, 5), rows), "CLI and library entry disagree"
    save("file_route", fam, names=names, route="cli", biotype=np.int32(1), n_anchors=np.int32(5), weight=np.float32(2.0), subm=subm.reshape(-1), scal=scal,
         rows=rows)


if __name__ == "__main__":
    main()
