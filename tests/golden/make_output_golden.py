"""Records tests/golden/out_*.npz: finished rows and the texts the reference writes from them.  Needs the compiled reference
(make -C oracle ref cli) and its sources; run from the repository root:

    python tests/golden/make_output_golden.py [REFERENCE_ROOT]        (default: $KALIGN_REF or /root/reference)

Through the reference's CLI (-f fasta | clu | msf on one input, -n 1), per case: names / name_off, rows (uint8 [n, alnlen],
parsed from the FASTA output), fasta / clu / msf (the three texts, uint8), title (the MSF file's basename), date (cut from the
MSF line: the one field that changes from run to run), biotype (0 protein, 1 DNA, as the case was made).
Through python-kalign/io.py, loaded by path, on the rows of the protein and the DNA case: fasta80 / fasta7 (write_fasta),
residue_conf (float32 [n, alnlen]) and column_conf (float32 [alnlen]) with sto_res / sto_col / sto_both (write_stockholm), and
sto_noids (both, ids=None).  out_pp.npz: a float32 sweep `values` and `chars`, _conf_to_pp_char of each.
Data only: no program text of the reference is stored."""
import importlib.util
import io
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.dirname(os.path.abspath(__file__))
CLI = os.path.join(ROOT, "oracle", "_ref", "kalign_ref")
PROT = "ACDEFGHIKLMNPQRSTVWY"
NUC = "ACGT"


def load_io(root):
    spec = importlib.util.spec_from_file_location("kalign_io_ref", os.path.join(root, "python-kalign", "io.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def pack(strs):
    bs = [s.encode() for s in strs]
    off = np.zeros(len(bs) + 1, np.int64)
    off[1:] = np.cumsum([len(b) for b in bs])
    return np.frombuffer(b"".join(bs), np.uint8).copy(), off


def family(rng, alphabet, n, lo, hi, p_sub=0.2, p_indel=0.05):
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
        out.append(bytes(s).decode())
    return out


def cli(seqs, names, title, flags):
    """the reference's CLI on one FASTA input, once per format: (rows, {format: text})"""
    texts = {}
    with tempfile.TemporaryDirectory() as tmp:
        inp = os.path.join(tmp, "in.fa")
        with open(inp, "w") as f:
            for n, s in zip(names, seqs):
                f.write(">%s\n%s\n" % (n, s))
        for fmt in ("fasta", "clu", "msf"):
            out = os.path.join(tmp, title)
            subprocess.run([CLI, "-i", inp, "-o", out, "-f", fmt, "-n", "1"] + flags, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            texts[fmt] = open(out, "rb").read()
            os.remove(out)
    got, rows = [], []
    for line in texts["fasta"].decode().split("\n")[:-1]:
        if line.startswith(">"):
            got.append(line[1:])
            rows.append("")
        else:
            rows[-1] += line
    assert got == list(names), (got, names)
    assert len(set(len(r) for r in rows)) == 1
    return rows, texts


def sweep():
    """the float32 values at which a PP byte changes, and their neighbours"""
    f = np.float32
    v = [f(0.0), f(-0.0), f(1.0), f(1e-42)]                      # (1e-42: a denormal)
    edges = [f(0.95)] + [f(k / 10) for k in range(1, 10)]
    for e in edges:
        v += [np.nextafter(e, f(0)), e, np.nextafter(e, f(1))]   # (the double edge lies between two of the three)
    return np.array(v, np.float32)


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("KALIGN_REF", "/root/reference")
    kio = load_io(ref_root)
    rng = np.random.default_rng(20261022)
    sw = sweep()
    np.savez_compressed(os.path.join(OUT, "out_pp.npz"), values=sw,
                        chars=np.frombuffer("".join(kio._conf_to_pp_char(float(x)) for x in sw).encode(), np.uint8))
    assert all(len(kio._conf_to_pp_char(float(x))) == 1 for x in sw)
    print("out_pp: %d values" % len(sw))

    prot = family(rng, PROT, 5, 70, 80)
    dna = family(rng, NUC, 4, 125, 135)
    same = "".join(rng.choice(list(PROT), size=120))
    cases = (("prot", prot, ["sp1", "a", "Q9XYZ1_HUMAN some protein, putative", "seq_four", "x5"], 0, ["--type", "protein"]),
             ("dna", dna, ["n1", "gene 2 (partial cds)", "n03", "n4"], 1, ["--type", "dna"]),
             ("w120", [same] * 3, ["r1", "row2", "r3"], 0, ["--type", "protein"]))
    # a family of one sequence cannot be recorded: the reference's front door refuses it ("Only 1 sequence was found",
    # msa_io.c:185) before any writer runs.  That it still does is checked here; the tests hold such a family against
    # tests/out_restate.py alone.
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "in.fa"), "w") as f:
            f.write(">lonely\n%s\n" % prot[0][:47])
        r = subprocess.run([CLI, "-i", os.path.join(tmp, "in.fa"), "-o", os.path.join(tmp, "one.msf"), "-f", "msf", "-n", "1", "--type", "protein"],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert r.returncode != 0 and b"Only 1 sequence was found" in r.stdout and not os.path.exists(os.path.join(tmp, "one.msf")), \
            "the reference now takes a family of one sequence: record it"
    for name, seqs, names, biotype, flags in cases:
        title = "%s.msf" % name
        rows, texts = cli(seqs, names, title, flags)
        if name == "w120":
            assert len(rows[0]) == 120, "the reference's alignment of equal sequences is no longer 120 wide"
        msf_line = texts["msf"].decode().split("\n")[2]
        date = msf_line.split("  ")[3]
        assert msf_line.startswith(" %s  MSF: " % title) and "  %s  Check: " % date in msf_line, msf_line
        d = dict(rows=np.array([np.frombuffer(r.encode(), np.uint8) for r in rows]), biotype=np.int32(biotype),
                 title=np.frombuffer(title.encode(), np.uint8), date=np.frombuffer(date.encode(), np.uint8))
        d["names"], d["name_off"] = pack(names)
        for k, v in texts.items():
            d[k] = np.frombuffer(v, np.uint8)
        if name in ("prot", "dna"):
            W = len(rows[0])
            for L in (80, 7):
                buf = io.StringIO()
                kio.write_fasta(rows, buf, ids=names, line_length=L)
                d["fasta%d" % L] = np.frombuffer(buf.getvalue().encode(), np.uint8)
            res = rng.random((len(rows), W)).astype(np.float32)
            col = rng.random(W).astype(np.float32)
            # the sweep at the first and last columns and across the row
            res[0, :len(sw)] = sw
            res[-1, -len(sw):] = sw[::-1]
            col[:len(sw)] = sw[::-1]
            col[-1], res[1, 0], res[1, -1] = sw[4], sw[5], sw[6]
            rl, cl = [[float(x) for x in r] for r in res], [float(x) for x in col]
            for key, kw in (("sto_res", dict(ids=names, residue_confidence=rl)), ("sto_col", dict(ids=names, column_confidence=cl)),
                            ("sto_both", dict(ids=names, residue_confidence=rl, column_confidence=cl)),
                            ("sto_noids", dict(residue_confidence=rl, column_confidence=cl))):
                buf = io.StringIO()
                kio.write_stockholm(rows, buf, **kw)
                d[key] = np.frombuffer(buf.getvalue().encode(), np.uint8)
            d["residue_conf"], d["column_conf"] = res, col
        np.savez_compressed(os.path.join(OUT, "out_%s.npz" % name), **d)
        print("out_%s: %d rows of %d, date %r, keys %s" % (name, len(rows), len(rows[0]), date, sorted(d)))


if __name__ == "__main__":
    main()
