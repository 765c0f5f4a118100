"""Writes tests/golden/ens_*.npz: the reference's ensemble consensus stage (lib/src/poar.c, consensus_msa.c) on members
whose residues disagree, run through oracle/_ref/libkalign_ref.so.

    python tests/golden/make_golden_ensemble.py        (needs oracle/_ref/libkalign_ref.so: `make -C oracle ref`)

Per case: the sequences, the members' rows (input order), the score of every member (score_alignment_poar), and per
min_support the consensus rows (build_consensus), their score and both confidence arrays (compute_residue_confidence);
plus the confidences of member 0's rows.  reference_stage() is also what tests/test_gpu_ensemble_stage.py uses for its
live randomized cases.

ens_real_*: members of the reference's own ensemble loop (kalign_run_seeded at the parameters of ensemble.c:32-76:
scaled gap penalties, a noisy guide tree from seed + k) on BB11001, BB30014 and a DNA set, every member also re-run with
KALIGN_REFINE_CONFIDENT, and kalign_ensemble's own output (rows, both confidence arrays) on the same input.  Self-check:
the stage restated over the POAR functions (scores, selection, consensus, refinement decision, confidence) reproduces
kalign_ensemble's output.
"""
import ctypes as C
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libkalign_ref.so")


class MsaSeq(C.Structure):                       # struct msa_seq, lib/src/msa_struct.h
    _fields_ = [("name", C.c_char_p), ("seq", C.c_void_p), ("s", C.c_void_p), ("gaps", C.c_void_p),
                ("confidence", C.POINTER(C.c_float)), ("rank", C.c_int), ("len", C.c_int), ("alloc_len", C.c_int)]


class Msa(C.Structure):                          # struct msa
    _fields_ = [("sequences", C.POINTER(C.POINTER(MsaSeq))), ("seq_distances", C.c_void_p),
                ("col_confidence", C.POINTER(C.c_float)), ("seq_weights", C.c_void_p), ("sip", C.c_void_p),
                ("nsip", C.c_void_p), ("plen", C.c_void_p), ("run_parallel", C.c_uint8), ("numseq", C.c_int),
                ("num_profiles", C.c_int), ("alloc_numseq", C.c_int), ("aligned", C.c_int), ("alnlen", C.c_int),
                ("letter_freq", C.c_int * 128), ("L", C.c_uint8), ("biotype", C.c_uint8), ("quiet", C.c_int),
                ("consistency_table", C.c_void_p)]


_lib = None


def available():
    return os.path.exists(REF_SO)


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(REF_SO)
        vp = C.c_void_p
        L.kalign_read_input.argtypes = [C.c_char_p, C.POINTER(C.POINTER(Msa)), C.c_int]
        L.kalign_free_msa.argtypes = [C.POINTER(Msa)]
        L.kalign_free_msa.restype = None
        L.poar_table_alloc.argtypes = [C.POINTER(vp), C.c_int]
        L.poar_table_free.argtypes = [vp]
        L.poar_table_free.restype = None
        L.pos_matrix_from_msa.argtypes = [C.POINTER(vp), C.POINTER(C.c_char_p), C.c_int, C.c_int]
        L.pos_matrix_free.argtypes = [vp]
        L.pos_matrix_free.restype = None
        L.extract_poars.argtypes = [vp, vp, C.c_int]
        L.score_alignment_poar.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(C.c_double)]
        L.build_consensus.argtypes = [vp, C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(Msa)]
        L.compute_residue_confidence.argtypes = [vp, C.POINTER(Msa)]
        L.kalign_run_seeded.argtypes = [C.POINTER(Msa), C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int,
                                        C.c_uint64, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_float]
        L.kalign_ensemble.restype = C.c_int
        L.kalign_ensemble.argtypes = [C.POINTER(Msa), C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float,
                                      C.c_uint64, C.c_int, C.c_char_p, C.c_int, C.c_float, C.c_float, C.c_int,
                                      C.c_float, C.c_int, C.c_float]
        _lib = L
    return _lib


def read_msa(seqs):
    """kalign_read_input on a FASTA of seqs (input order)"""
    L = lib()
    with tempfile.NamedTemporaryFile("w", suffix=".fa", delete=False) as f:
        for i, s in enumerate(seqs):
            f.write(">s%d\n%s\n" % (i, s))
        path = f.name
    m = C.POINTER(Msa)()
    try:
        assert L.kalign_read_input(path.encode(), C.byref(m), 1) == 0, "kalign_read_input failed"
    finally:
        os.unlink(path)
    return m


def _rows_ptrs(rows):
    bufs = [C.create_string_buffer(r.encode() if isinstance(r, str) else bytes(r)) for r in rows]
    arr = (C.c_char_p * len(rows))(*[C.cast(b, C.c_char_p) for b in bufs])
    return arr, bufs


class Table:
    """a POAR table filled from member rows (extract_poars per member, as kalign_ensemble's loop does)"""

    def __init__(self, members):
        L = lib()
        self.n = len(members[0])
        self.runs = len(members)
        self.t = C.c_void_p()
        assert L.poar_table_alloc(C.byref(self.t), self.n) == 0
        for k, rows in enumerate(members):
            pm = self._pm(rows)
            assert L.extract_poars(self.t, pm, k) == 0
            L.pos_matrix_free(pm)

    def _pm(self, rows):
        arr, _keep = _rows_ptrs(rows)
        pm = C.c_void_p()
        assert lib().pos_matrix_from_msa(C.byref(pm), arr, self.n, len(rows[0])) == 0
        return pm

    def score(self, rows):
        pm = self._pm(rows)
        v = C.c_double()
        assert lib().score_alignment_poar(self.t, pm, self.n, self.runs, C.byref(v)) == 0
        lib().pos_matrix_free(pm)
        return v.value

    def consensus(self, seqs, min_support):
        L = lib()
        m = read_msa(seqs)
        lens = (C.c_int * self.n)(*[m.contents.sequences[i].contents.len for i in range(self.n)])
        assert L.build_consensus(self.t, lens, self.n, min_support, m) == 0
        w = m.contents.alnlen
        rows = [C.string_at(m.contents.sequences[i].contents.seq, w).decode() for i in range(self.n)]
        L.kalign_free_msa(m)
        return rows

    def confidence(self, seqs, rows):
        """compute_residue_confidence on an msa whose rows are `rows`"""
        L = lib()
        libc = C.CDLL(None)
        libc.malloc.restype = C.c_void_p
        libc.malloc.argtypes = [C.c_size_t]
        libc.free.argtypes = [C.c_void_p]
        m = read_msa(seqs)
        w = len(rows[0])
        for i, r in enumerate(rows):
            sq = m.contents.sequences[i].contents
            p = libc.malloc(w + 1)
            C.memmove(p, (r.encode() if isinstance(r, str) else bytes(r)) + b"\0", w + 1)
            libc.free(sq.seq)
            sq.seq = p
            sq.len = w
        m.contents.alnlen = w
        assert L.compute_residue_confidence(self.t, m) == 0
        res = np.array([[m.contents.sequences[i].contents.confidence[c] for c in range(w)] for i in range(self.n)], np.float32)
        col = np.array([m.contents.col_confidence[c] for c in range(w)], np.float32)
        L.kalign_free_msa(m)
        return res, col

    def close(self):
        if self.t:
            lib().poar_table_free(self.t)
            self.t = None


def reference_stage(seqs, members, min_supports):
    """the reference's stage on these members: dict of arrays (what an ens_*.npz holds)"""
    t = Table(members)
    out = dict(seqs=np.array(seqs), members=np.array(members), min_supports=np.array(min_supports, np.int32))
    out["scores"] = np.array([t.score(r) for r in members], np.float64)
    r0, c0 = t.confidence(seqs, members[0])
    out["m0_res_conf"], out["m0_col_conf"] = r0, c0
    for m in min_supports:
        rows = t.consensus(seqs, int(m))
        out["cons%d" % m] = np.array(rows)
        out["cons%d_score" % m] = np.float64(t.score(rows))
        rc, cc = t.confidence(seqs, rows)
        out["cons%d_res_conf" % m], out["cons%d_col_conf" % m] = rc, cc
    t.close()
    return out


# ---------------------------------------------------------------------------------------------------------------------
# synthetic members: one base alignment, each member moves residues across the gap runs next to them
# ---------------------------------------------------------------------------------------------------------------------
def synthetic(n, length, n_runs, seed, alphabet="ACDEFGHIKLMNPQRSTVWYacdefghiklmnpqrstvwyX", gap_frac=0.25, moves=6):
    rng = np.random.default_rng(seed)
    seqs = []
    for _ in range(n):
        L = int(rng.integers(max(1, length // 2), length + 1))
        seqs.append("".join(rng.choice(list(alphabet), L)))
    width = int(max(len(s) for s in seqs) * (1 + gap_frac)) + 2
    base = []
    for s in seqs:
        cols = np.sort(rng.choice(width, len(s), replace=False))
        row = np.full(width, ord("-"), np.uint8)
        row[cols] = np.frombuffer(s.encode(), np.uint8)
        base.append(row)
    members = []
    for k in range(n_runs):
        rows = []
        for row in base:
            r = row.copy()
            for _ in range(int(rng.integers(0, moves + 1))):
                c = int(rng.integers(0, width - 1))
                a, b = r[c] != ord("-"), r[c + 1] != ord("-")
                if a != b:                       # a residue next to a gap: move it across
                    r[c], r[c + 1] = r[c + 1], r[c]
            rows.append(r.tobytes().decode().replace("-", "-" if k % 2 else "."))
        members.append(rows)
    return seqs, members


CASES = [  # name, n, length, runs, seed, alphabet, min_supports
    ("syn2", 12, 40, 2, 1, None, [1, 2]),
    ("syn3", 16, 50, 3, 2, None, [1, 2, 3]),
    ("syn8", 24, 60, 8, 3, None, list(range(1, 9))),
    ("syn32", 10, 30, 32, 4, None, [1, 2, 3, 8, 11, 16, 24, 32]),
    ("syn8dna", 20, 80, 8, 5, "ACGTNacgtn", [1, 3, 5, 8]),
]


# ensemble.c:32-45: (gpo, gpe, tgpe) multipliers and tree noise of member k (k % 12; member 0 runs the defaults)
RUN_PARAMS = [(1.0, 1.0, 1.0, 0.0), (0.5, 1.5, 0.8, 0.20), (1.5, 0.5, 1.2, 0.20), (0.7, 0.7, 0.5, 0.25), (1.4, 1.4, 1.5, 0.25),
              (0.8, 1.2, 1.0, 0.30), (1.3, 0.8, 0.7, 0.30), (0.6, 1.0, 1.3, 0.15), (1.0, 0.6, 0.6, 0.15), (1.8, 1.0, 1.0, 0.35),
              (1.0, 1.8, 1.8, 0.35), (0.4, 0.4, 0.3, 0.20)]


def member_params(base, k, seed):
    """resolve_run_params (ensemble.c:55-76): (gpo, gpe, tgpe) in binary32, tree seed, noise sigma"""
    if k == 0:
        return tuple(np.float32(x) for x in base), 0, 0.0
    g, e, t, noise = RUN_PARAMS[k % len(RUN_PARAMS)]
    return (np.float32(base[0]) * np.float32(g), np.float32(base[1]) * np.float32(e), np.float32(base[2]) * np.float32(t)), \
        seed + k, noise


def base_penalties(seqs, type_=-1):
    """the default gap penalties aln_param_init resolves for this input (what kalign_ensemble scales)"""
    sys.path.insert(0, ROOT)
    from oracle import refdrv
    j = refdrv.RefJob(seqs, type_=type_)
    out = (j.gpo, j.gpe, j.tgpe)
    j.close()
    return out


def reference_member(seqs, k, seed, base, refine=0, type_=-1):
    """member k of kalign_ensemble's loop (ensemble.c:286-315): the reference's kalign_run_seeded at the member's
    parameters (fast mode, no sequence weights); rows in input order"""
    L = lib()
    (g, e, t), tseed, noise = member_params(base, k, seed)
    m = read_msa(seqs)
    rc = L.kalign_run_seeded(m, 1, 8 if type_ < 0 else type_, g, e, t, refine, 0, tseed, noise, 0.0, -1.0, 0.0, 0, 2.0)
    assert rc == 0, "kalign_run_seeded failed"
    n, w = m.contents.numseq, m.contents.alnlen
    rows = [C.string_at(m.contents.sequences[i].contents.seq, w).decode() for i in range(n)]
    L.kalign_free_msa(m)
    return rows


def kalign_ensemble(seqs, n_runs, seed, min_support=0, type_=-1):
    """the reference's kalign_ensemble (fast mode: no anchors, no realignment; members unrefined): (rows, residue
    confidence, column confidence), rows in input order"""
    L = lib()
    m = read_msa(seqs)
    rc = L.kalign_ensemble(m, 1, 8 if type_ < 0 else type_, n_runs, -1.0, -1.0, -1.0, seed, min_support, None, 0, 0.0, -1.0,
                           0, -1.0, 0, 2.0)
    assert rc == 0, "kalign_ensemble failed"
    n, w = m.contents.numseq, m.contents.alnlen
    rows = [C.string_at(m.contents.sequences[i].contents.seq, w).decode() for i in range(n)]
    res = np.array([[m.contents.sequences[i].contents.confidence[c] for c in range(w)] for i in range(n)], np.float32)
    col = np.array([m.contents.col_confidence[c] for c in range(w)], np.float32)
    L.kalign_free_msa(m)
    return rows, res, col


def select(scores):
    """score_alignments' choice (ensemble.c:121-127)"""
    best = 0
    for k in range(1, len(scores)):
        if scores[k] > scores[best] and scores[k] > scores[0] * 1.05:
            best = k
    return best


def reference_finish(seqs, members, rerun_refined):
    """kalign_ensemble's tail (ensemble.c:341-497, automatic min_support) restated over the reference's POAR functions:
    (rows, residue confidence, column confidence, decision)"""
    n_runs = len(members)
    auto = max(2, (n_runs + 2) // 3)
    t = Table(members)
    scores = [t.score(r) for r in members]
    best = select(scores)
    cons = t.consensus(seqs, auto)
    if t.score(cons) > scores[best]:
        want, decision = cons, "consensus"
    else:
        refined = rerun_refined(best)
        if t.score(refined) > scores[best]:
            want, decision = refined, "refined"
        else:
            want, decision = members[best], "selection"
    res, col = t.confidence(seqs, want)
    t.close()
    return want, res, col, decision


def real_case(seqs, n_runs, seed, type_=-1):
    """members, refined members and kalign_ensemble's output; the self-check; the POAR stage's arrays"""
    base = base_penalties(seqs, type_)
    members = [reference_member(seqs, k, seed, base, type_=type_) for k in range(n_runs)]
    refined = [reference_member(seqs, k, seed, base, refine=2, type_=type_) for k in range(n_runs)]
    auto = max(2, (n_runs + 2) // 3)
    out = reference_stage(seqs, members, sorted({1, auto, n_runs}))
    ens_rows, ens_res, ens_col = kalign_ensemble(seqs, n_runs, seed, type_=type_)
    # self-check: kalign_ensemble's tail restated over the POAR functions gives kalign_ensemble's output
    want, res, col, decision = reference_finish(seqs, members, lambda k: refined[k])
    assert want == ens_rows, "members / POAR stage do not reproduce kalign_ensemble"
    assert np.array_equal(res, ens_res) and np.array_equal(col, ens_col), "confidences differ from kalign_ensemble"
    out["members"] = np.array(members)
    out["refined"] = np.array(refined)
    out["ens_rows"], out["ens_res_conf"], out["ens_col_conf"] = np.array(ens_rows), ens_res, ens_col
    out["seed"] = np.int64(seed)
    return out, decision


def read_fasta(path):
    seqs, cur = [], None
    for line in open(path):
        line = line.strip()
        if line.startswith(">"):
            if cur is not None:
                seqs.append(cur)
            cur = ""
        elif cur is not None:
            cur += line
    if cur is not None:
        seqs.append(cur)
    return seqs


def real_inputs():
    sys.path.insert(0, ROOT)
    from kalign_amd import synth
    return [("bb11001", read_fasta(os.path.join(HERE, "data", "BB11001.tfa")), -1),
            ("bb30014", read_fasta(os.path.join(HERE, "data", "BB30014.tfa")), -1),
            ("dna40", synth.dssim(40, 150, dna=True, seed=3), -1)]


def main():
    assert available(), "build oracle/_ref first: make -C oracle ref"
    for name, seqs, type_ in real_inputs():
        for runs in (3, 8):
            out, decision = real_case(seqs, runs, 42, type_)
            np.savez_compressed(os.path.join(HERE, "ens_real_%s_r%d.npz" % (name, runs)), **out)
            print("ens_real_%s_r%d: %d seqs, %d members, kalign_ensemble took the %s; self-check passed"
                  % (name, runs, len(seqs), runs, decision))
    for name, n, length, runs, seed, alpha, mins in CASES:
        kw = {} if alpha is None else dict(alphabet=alpha)
        seqs, members = synthetic(n, length, runs, seed, **kw)
        out = reference_stage(seqs, members, mins)
        np.savez_compressed(os.path.join(HERE, "ens_%s.npz" % name), **out)
        print("ens_%s: %d x ~%d, %d members, scores %s" % (name, n, length, runs, np.round(out["scores"], 3).tolist()))


if __name__ == "__main__":
    sys.exit(main())
