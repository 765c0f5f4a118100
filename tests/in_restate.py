"""A numpy restatement of the input stage (include/kalign_amd.h, the input stage): the rule for a byte, the histogram,
the checksum, the aligned status, the order, detection and the three encodings -- written from the rule's text, sharing
nothing with the library.  tests/test_input_host.py holds it to the goldens recorded from the reference
(tests/golden/in_*.npz), tests/test_gpu_input.py holds the library to it."""
import glob
import math
import os

import numpy as np

SEQ = ("residues", "gap_characters", "dropped", "checksum")
FAM = ("biotype", "aligned", "min_len", "max_len", "no_code")
NAME_LEN = 256


def raw(s):
    return np.frombuffer(s.encode("latin-1") if isinstance(s, str) else bytes(s), np.uint8)


def is_letter(b):
    return ((b >= 65) & (b <= 90)) | ((b >= 97) & (b <= 122))


def is_punct(b):
    return ((b >= 33) & (b <= 47)) | ((b >= 58) & (b <= 64)) | ((b >= 91) & (b <= 96)) | ((b >= 123) & (b <= 126))


def scan(s):
    """one sequence -> dict: residues (the letters as given, uint8), the four counts of SEQ, bad (offset of the first byte
    >= 128, or -1)"""
    b = raw(s)
    let, pun, high = is_letter(b), is_punct(b), b >= 128
    res = b[let]
    chk = 0
    for i, c in enumerate(res.tolist()):                 # (the reference's loop, a remainder per step)
        chk = (chk + (i % 57 + 1) * (c - 32 if c >= 97 else c)) % 10000
    return dict(letters=res, residues=len(res), gap_characters=int(pun.sum()), dropped=int((~let & ~pun & ~high).sum()),
                checksum=chk, bad=int(np.argmax(high)) if high.any() else -1)


def histogram(family):
    h = np.zeros(128, np.int64)
    for s in family:
        b = raw(s)
        h += np.bincount(b[b < 128], minlength=128)[:128]
    return h


def detect(freq):
    """0 protein, 1 DNA, None when the two sums are equal"""
    dna = [math.log(0.0001 * 1.0 / 116.0)] * 128
    prot = [math.log(0.0001 * 1.0 / 88.0)] * 128
    for c in b"acgtunACGTUN":
        dna[c] = math.log(0.9999 * 1.0 / 12.0)
    for c in b"acdefghiklmnpqrstvwyACDEFGHIKLMNPQRSTVWY":
        prot[c] = math.log(0.9999 * 1.0 / 40.0)
    d = p = 0.0
    for i in range(128):
        if freq[i]:
            d += dna[i] * float(freq[i])
            p += prot[i] * float(freq[i])
    return None if d == p else (1 if d > p else 0)


def status(residues, gaps):
    """1 unaligned, 2 aligned, 3 unknown"""
    total = np.asarray(residues, np.int64) + np.asarray(gaps, np.int64)
    same = total.min() == total.max()
    if int(np.sum(gaps)):
        return 2 if same else 3
    return 3 if same else 1


def _name_key(n):
    n = bytes(n)[:NAME_LEN]
    z = n.find(b"\0")
    return n if z < 0 else n[:z]


def order(residues, names=None):
    """sorted position -> input index: more residues first, then the lower name (bytes compare as unsigned, a shorter name
    that is a prefix comes first: strncmp), then the lower index"""
    idx = list(range(len(residues)))
    key = (lambda i: (-int(residues[i]), i)) if names is None else (lambda i: (-int(residues[i]), _name_key(raw(names[i]).tobytes()), i))
    return np.array(sorted(idx, key=key), np.int32)


def _table(letters, merges, alias, code_of_alias):
    t = np.full(128, -1, np.int64)
    for k, c in enumerate(letters):
        t[ord(c)] = k
    for x, y in merges:
        t[ord(x)] = t[ord(y)] = min(t[ord(x)], t[ord(y)])
    if alias:
        t[ord(alias)] = t[ord(code_of_alias)]
    used = sorted(set(int(v) for v in t[64:96] if v >= 0))
    dense = {v: k for k, v in enumerate(used)}
    for b in range(64, 96):
        if t[b] >= 0:
            t[b] = t[b + 32] = dense[int(t[b])]
    return t.astype(np.int8)


def tables():
    """int8 [3, 128]: nucleotides, reduced protein, protein; -1: no code"""
    nuc = _table("ACGTUNRYSWKMBDHV", [("U", "T")] + [("N", c) for c in "RYSWKMBDHV"], None, None)
    red = _table("ACDEFGHIKLMNPQRSTVWYBZX", [("L", "M"), ("I", "V"), ("K", "R"), ("E", "Q"), ("A", "S"), ("A", "T"), ("S", "T"), ("N", "D"),
                                             ("F", "Y"), ("B", "N"), ("B", "D"), ("Z", "E"), ("Z", "Q")], "U", "C")
    prot = _table("ARNDCQEGHILKMFPSTWYVBZX", [], "U", "X")
    return np.stack([nuc, red, prot])


def family(fam, names=None, biotype=-1):
    """everything the stage says about one family: dict of seqs (int32 [n, 4], input order), fam (dict of FAM), freq, order,
    and the three planes as lists of uint8 arrays in sorted order.  Raises ValueError as the stage refuses."""
    sc = [scan(s) for s in fam]
    for i, r in enumerate(sc):
        if r["bad"] >= 0:
            raise ValueError("sequence %d: byte 0x%02x at offset %d" % (i, raw(fam[i])[r["bad"]], r["bad"]))
    for i, r in enumerate(sc):
        if r["residues"] == 0:
            raise ValueError("sequence %d has no residue" % i)
    freq = histogram(fam)
    bt = biotype if biotype >= 0 else detect(freq)
    if bt is None:
        raise ValueError("could not determine the alphabet")
    res = np.array([r["residues"] for r in sc], np.int32)
    gaps = np.array([r["gap_characters"] for r in sc], np.int32)
    o = order(res, names)
    T = tables()
    t_tree, t_aln = (T[0], T[0]) if bt == 1 else (T[1], T[2])
    letters = [sc[i]["letters"] for i in o]
    no_code = sum(int((t_aln[x] < 0).sum()) for x in letters)
    return dict(seqs=np.array([[r[k] for k in SEQ] for r in sc], np.int32),
                fam=dict(biotype=bt, aligned=status(res, gaps), min_len=int(res.min()), max_len=int(res.max()), no_code=no_code),
                freq=freq, order=o, letters=letters,
                tree_codes=[np.maximum(t_tree[x], 0).astype(np.uint8) for x in letters],
                codes=[np.maximum(t_aln[x], 0).astype(np.uint8) for x in letters])


class InGolden:
    """one tests/golden/in_*.npz: the input (seqs, names or None) and what the reference made of it (see
    tests/golden/make_input_golden.py for the fields)"""

    def __init__(self, path):
        z = np.load(path)
        self.name = os.path.basename(path)[3:-4]
        self.z = {k: z[k] for k in z.files}
        off = self.z["seq_off"]
        self.seqs = [self.z["text"][off[i]:off[i + 1]].tobytes() for i in range(len(off) - 1)]
        self.names = None
        if "name_off" in self.z:
            o = self.z["name_off"]
            self.names = [self.z["names"][o[i]:o[i + 1]].tobytes() for i in range(len(o) - 1)]

    def has(self, k):
        return k in self.z

    def __getattr__(self, k):
        try:
            return self.__dict__["z"][k]
        except KeyError:
            raise AttributeError(k)

    def split(self, flat):
        """a flat plane of the reference (sorted order) as one array per sequence"""
        o = np.concatenate([[0], np.cumsum(self.z["lens"])])
        return [flat[o[i]:o[i + 1]] for i in range(len(o) - 1)]

    def row_bytes(self):
        return [r.tobytes() for r in self.z["rows"]]


def goldens(golden_dir):
    return [InGolden(p) for p in sorted(glob.glob(os.path.join(golden_dir, "in_*.npz")))]
