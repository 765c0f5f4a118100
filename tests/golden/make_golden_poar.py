"""Writes tests/golden/poar_*.npz: the POAR file of the members of every ens_*.npz (make_golden_ensemble.py), as the
reference's poar_table_write writes it (lib/src/poar.c:203-252).

    python tests/golden/make_golden_poar.py        (needs oracle/_ref/libkalign_ref.so: `make -C oracle ref`)

Per case: `size` and `sha256` of the file, `n_entries` per pair (uint32, file order), and the file itself (`image`, uint8)
where it is at most 100 KB.  Self-checks: the numpy restatement (tests/poar_restate.py) equals the reference's bytes; for
ens_real_*, kalign_ensemble(save_poar_path=...) at the stored seed writes the same bytes; kalign_consensus_from_poar on the
file returns, at every stored min_support, the stored consensus rows and both confidence arrays.
"""
import ctypes as C
import glob
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden_ensemble as mg  # noqa: E402
import poar_restate  # noqa: E402

IMAGE_LIMIT = 100 * 1024


def lib():
    L = mg.lib()
    L.poar_table_write.argtypes = [C.c_void_p, C.c_char_p]
    L.poar_table_read.argtypes = [C.POINTER(C.c_void_p), C.c_char_p]
    L.kalign_consensus_from_poar.argtypes = [C.POINTER(mg.Msa), C.c_char_p, C.c_int]
    return L


def reference_image(members):
    """poar_table_write of a table filled by extract_poars member by member"""
    t = mg.Table(members)
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "t.poar")
        assert lib().poar_table_write(t.t, p.encode()) == 0
        data = open(p, "rb").read()
    t.close()
    return data


def reference_read(path):
    """poar_table_read alone (timing); frees the table"""
    t = C.c_void_p()
    assert lib().poar_table_read(C.byref(t), path.encode()) == 0
    lib().poar_table_free(t)


def consensus_from_poar(seqs, path, min_support):
    """the reference's kalign_consensus_from_poar: (rows, residue confidence, column confidence), input order"""
    L = lib()
    m = mg.read_msa(seqs)
    assert L.kalign_consensus_from_poar(m, path.encode(), int(min_support)) == 0, "kalign_consensus_from_poar failed"
    n, w = m.contents.numseq, m.contents.alnlen
    rows = [C.string_at(m.contents.sequences[i].contents.seq, w).decode() for i in range(n)]
    res = np.array([[m.contents.sequences[i].contents.confidence[c] for c in range(w)] for i in range(n)], np.float32)
    col = np.array([m.contents.col_confidence[c] for c in range(w)], np.float32)
    L.kalign_free_msa(m)
    return rows, res, col


def ensemble_saved_image(seqs, n_runs, seed):
    """the file kalign_ensemble(save_poar_path=...) writes (fast mode, as make_golden_ensemble.kalign_ensemble)"""
    L = lib()
    m = mg.read_msa(seqs)
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "e.poar")
        rc = L.kalign_ensemble(m, 1, 8, n_runs, -1.0, -1.0, -1.0, seed, 0, p.encode(), 0, 0.0, -1.0, 0, -1.0, 0, 2.0)
        assert rc == 0, "kalign_ensemble failed"
        data = open(p, "rb").read()
    L.kalign_free_msa(m)
    return data


def main():
    assert mg.available(), "build oracle/_ref first: make -C oracle ref"
    names = sorted(os.path.basename(f)[4:-4] for f in glob.glob(os.path.join(HERE, "ens_*.npz")))
    for name in names:
        z = np.load(os.path.join(HERE, "ens_%s.npz" % name))
        seqs = [str(s) for s in z["seqs"]]
        members = [["".join(r) for r in m] for m in z["members"]]
        image = reference_image(members)
        assert poar_restate.poar_image(members) == image, "%s: the restatement differs from poar_table_write" % name
        if name.startswith("real_"):
            assert ensemble_saved_image(seqs, len(members), int(z["seed"])) == image, "%s: kalign_ensemble saved another table" % name
        with tempfile.TemporaryDirectory() as d:
            p = os.path.join(d, "t.poar")
            open(p, "wb").write(image)
            for m in z["min_supports"]:
                rows, res, col = consensus_from_poar(seqs, p, int(m))
                assert rows == [str(x) for x in z["cons%d" % m]], (name, int(m))
                assert np.array_equal(res, z["cons%d_res_conf" % m]) and np.array_equal(col, z["cons%d_col_conf" % m]), (name, int(m))
        out = dict(size=np.int64(len(image)), sha256=np.array(poar_restate.sha256(image)),
                   n_entries=poar_restate.pair_counts(image, len(seqs)))
        if len(image) <= IMAGE_LIMIT:
            out["image"] = np.frombuffer(image, np.uint8)
        np.savez_compressed(os.path.join(HERE, "poar_%s.npz" % name), **out)
        print("poar_%s: %d bytes, %d entries, image %s; self-checks passed"
              % (name, len(image), int(out["n_entries"].sum()), "stored" if "image" in out else "pinned by hash"))


if __name__ == "__main__":
    sys.exit(main())
