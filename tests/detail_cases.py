"""The families of the detail tests (test_detail_inputs.py, test_gpu_compare_detail.py): the stored (reference, test)
pairs of tests/golden/cmp_*.npz with their recorded column correctness (col_*.npz), and the seeded edge batch."""
import glob
import os

import numpy as np

from cmp_cases import family
from util import GOLDEN

EDGE_N = [2, 3, 16, 17, 32, 33, 47]        # the KA_CMP_TI / KA_CMP_TJ boundaries
DEEP_N = [65, 130]                         # at width 9: the column pass strides its 64 lanes over the rows; 3 and 5 j-tiles
EDGE_W = [1, 7, 8, 9, 15, 16, 17, 63, 64, 65]


def stored_pairs():
    """[(case name, test index, reference rows, test rows, recorded flags)] of the 28 stored pairs, rows paired by name"""
    from kalign_amd import compare as kc
    out = []
    for path in sorted(glob.glob(os.path.join(GOLDEN, "cmp_*.npz"))):
        name = os.path.basename(path)[4:-4]
        z = np.load(path)
        flags = np.load(os.path.join(GOLDEN, "col_%s.npz" % name))["correct"]
        names = [str(n) for n in z["names"]]
        tnames = [str(n) for n in z["test_names"]] if "test_names" in z.files else names
        assert flags.shape == (len(z["tests"]), len(str(z["tests"][0][0]))) and flags.dtype == np.uint8
        for k, t in enumerate(z["tests"]):
            r, tt = kc.pair_rows(list(zip(names, (str(x) for x in z["ref"]))), list(zip(tnames, (str(x) for x in t))))
            out.append((name, k, r, tt, flags[k]))
    return out


def moved(rng, ref, share, extra=0):
    """the test of a family that is nearly right: the reference's rows with `share` of the residues moved by one column
    into a gap next to them (inside their gap run: the letters keep their order), then `extra` all-gap columns put in at
    random places"""
    a = np.frombuffer(b"".join(ref), np.uint8).reshape(len(ref), -1).copy()
    W = a.shape[1]
    gap = ord("-")
    for row in a:
        for c in rng.permutation(W):
            if row[c] == gap or rng.rand() >= share:
                continue
            n = c + (1 if rng.rand() < 0.5 else -1)
            if 0 <= n < W and row[n] == gap:
                row[n], row[c] = row[c], gap
    for _ in range(extra):
        a = np.insert(a, rng.randint(0, a.shape[1] + 1), gap, axis=1)
    return [r.tobytes() for r in a]


def near_family(rng, N, W, extra=0, fill=0.6):
    """(reference rows, test rows): N random sequences placed in W columns, and moved() of them -- the share chosen so
    that about half of the columns keep all their residues in place: (1 - share) ** (N * fill) = 1 / 2"""
    r, _ = family(rng, N, W, W)
    share = 1.0 - 0.5 ** (1.0 / max(1.0, N * fill))
    return r, moved(rng, r, share, extra)


def edge_batch():
    """(refs, tests, notes): the edge batch of the detail tests, seeded; notes names the families a test looks for"""
    rng = np.random.RandomState(2027)
    refs, tests, notes = [], [], {}

    def add(pair, note=None):
        if note:
            notes.setdefault(note, []).append(len(refs))
        refs.append(pair[0])
        tests.append(pair[1])

    # the tile boundaries, with widths at the pad boundaries, the test wider and narrower than its reference
    for k, N in enumerate(EDGE_N):
        for j in range(3):
            add(family(rng, N, EDGE_W[(3 * k + j) % 10], EDGE_W[(7 * k + 3 * j + 4) % 10]))
    for WR, WT in ((1, 65), (65, 1), (1, 1)):
        add(family(rng, 3, WR, WT))
    for N in DEEP_N:
        add(family(rng, N, 9, 9), "deep")
    # 40 x 600 / 610: (WRp + WTp) * 2 bytes * 32 rows > 64 KiB, so TJ < 32 and two j-tiles
    add(near_family(rng, 40, 600, extra=10), "lds")
    # six consecutive families of width 1 - 3: a chunk of the column pass spans several jobs
    for q in range(6):
        add(family(rng, 2 + q % 2, 1 + q % 3, 1 + (q + 1) % 3), "narrow")
    # an all-gap reference column; an all-gap test column (the two roles of family() swapped); a sequence without residues
    add(family(rng, 17, 64, 63, free=9), "gap_ref_col")
    t, r = family(rng, 9, 24, 20, free=3)
    add((r, t), "gap_test_col")
    add(family(rng, 5, 17, 15, zero=True), "no_residues")
    # for every N a family whose test is nearly its reference: both flag values at k >= 2
    for q, N in enumerate(EDGE_N):
        add(near_family(rng, N, (63, 64, 65)[q % 3], extra=q % 3), "near")
    for N in DEEP_N:
        add(near_family(rng, N, 9, fill=0.75), "near")
    return refs, tests, notes
