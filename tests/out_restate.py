"""The four output formats of the output stage (ka_out_fam) restated in Python, a loop over rows and lines as the reference's
writers are: write_msa_fasta / write_msa_clu / write_msa_msf (lib/src/msa_io.c) and kalign.io.write_fasta /
write_stockholm (python-kalign/io.py).  Rows and names are bytes; every function returns the text of one family as bytes.
The goldens (tests/golden/out_*.npz, tests/golden/make_output_golden.py) pin it to the reference byte for byte."""
import glob
import os

import numpy as np

BLOCK = 60
MSF_BANNER = {0: b"!!NA_MULTIPLE_ALIGNMENT 1.0", 1: b"!!NA_MULTIPLE_ALIGNMENT 1.0"}    # what the reference's CLI writes after a run
MSF_TYPE = {0: b"N", 1: b"N"}


def default_names(n):
    return [b"seq%d" % i for i in range(n)]


def fasta(rows, names=None, line_length=60):
    names = default_names(len(rows)) if names is None else names
    out = []
    for name, row in zip(names, rows):
        out.append(b">" + name + b"\n")
        for i in range(0, len(row), line_length):
            out.append(row[i:i + line_length] + b"\n")
    return b"".join(out)


def fasta_size(widths_names, line_length):
    """closed form: widths_names is [(W, [name lengths])] of one family"""
    W, lens = widths_names
    return sum(1 + n + 1 + W + (W + line_length - 1) // line_length for n in lens)


def blocks(rows, names):
    """the blocks Clustal and MSF share: per block one line per row -- the name padded to the longest name + 5, up to 60
    bytes of the row -- then the separator line, a newline printed with a newline"""
    pad = max(len(n) for n in names) + 5
    W = len(rows[0])
    out = []
    for b in range(max(1, (W + BLOCK - 1) // BLOCK)):
        for name, row in zip(names, rows):
            out.append(name + b" " * (pad - len(name)) + row[BLOCK * b:BLOCK * (b + 1)] + b"\n")
        out.append(b"\n\n")
    return b"".join(out)


def blocks_size(W, lens):
    N, pad = len(lens), max(lens) + 5
    nb = max(1, (W + BLOCK - 1) // BLOCK)
    return (nb - 1) * (N * (pad + BLOCK + 1) + 2) + N * (pad + W - BLOCK * (nb - 1) + 1) + 2


def clustal(rows, names=None, header=b""):
    names = default_names(len(rows)) if names is None else names
    return header + b"\n" + b"\n" + blocks(rows, names)


def gcg_checksum(seq):
    chk = 0
    for i, c in enumerate(seq.upper()):
        chk = (chk + (i % 57 + 1) * c) % 10000
    return chk


def msf_records(rows, gap=b"-"):
    """per row (characters, GCGchecksum of the first `characters` bytes of the aligned row), and the family's check"""
    recs = []
    for row in rows:
        n = len(row) - row.count(gap)
        # (bytes.upper touches a-z alone)
        recs.append((n, gcg_checksum(row[:n])))
    check = 0
    for _, c in recs:
        check = (check + c) % 10000
    return recs, check


def msf(rows, names, title, biotype, date, gap=b"-"):
    names = default_names(len(rows)) if names is None else names
    recs, check = msf_records(rows, gap)
    width = max(len(n) for n in names)
    length = recs[0][0]
    out = [MSF_BANNER[biotype], b"",
           b" %s  MSF: %d  Type: %s  %s  Check: %d  .." % (title, length, MSF_TYPE[biotype], date, check), b""]
    for name, (_, c) in zip(names, recs):
        out.append(b" Name: %s  Len:  %5d  Check: %4d  Weight: 1.00" % (name + b" " * (width - len(name)), length, c))
    out += [b"", b"//", b""]
    return b"".join(x + b"\n" for x in out) + blocks(rows, names)


def pp_char(v):
    """kalign.io._conf_to_pp_char on a float32's value; None for a NaN or a value outside [0, 1]"""
    v = float(np.float32(v))
    if not (0.0 <= v <= 1.0):
        return None
    return b"*" if v >= 0.95 else b"%d" % int(v * 10)


def stockholm(rows, names=None, residue_conf=None, column_conf=None):
    names = default_names(len(rows)) if names is None else names
    max_id = max(len(n) for n in names)
    out = [b"# STOCKHOLM 1.0\n"]
    for k, (name, row) in enumerate(zip(names, rows)):
        label = name + b" " * (max_id - len(name))
        out.append(label + b"   " + row + b"\n")
        if residue_conf is not None:
            pp = b"".join(b"." if ch in b"-." else pp_char(v) for ch, v in zip(row, residue_conf[k]))
            out.append(b"#=GR " + label + b" PP " + pp + b"\n")
    if column_conf is not None:
        out.append(b"#=GC " + b"PP_cons".ljust(max(max_id, 7)) + b"   " + b"".join(pp_char(v) for v in column_conf) + b"\n")
    out.append(b"//\n")
    return b"".join(out)


def stockholm_size(W, lens, has_res, has_col):
    N, m = len(lens), max(lens)
    return 16 + N * ((m + 3 + W + 1) + ((5 + m + 4 + W + 1) if has_res else 0)) + ((5 + max(m, 7) + 3 + W + 1) if has_col else 0) + 3


class Case:
    """one tests/golden/out_*.npz: rows and names as lists of bytes, the recorded texts as bytes"""

    def __init__(self, path):
        self.name = os.path.basename(path)[4:-4]
        self.z = np.load(path)
        z = self.z
        self.rows = [r.tobytes() for r in z["rows"]] if "rows" in z.files else None
        if "names" in z.files:
            n, o = z["names"].tobytes(), z["name_off"]
            self.names = [n[o[i]:o[i + 1]] for i in range(len(o) - 1)]

    def has(self, k):
        return k in self.z.files

    def text(self, k):
        return self.z[k].tobytes()


def goldens(golden_dir):
    return [Case(p) for p in sorted(glob.glob(os.path.join(golden_dir, "out_*.npz")))]
