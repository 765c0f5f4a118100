"""Seeded jobs for the streamed-bonus kernels (`--consistency K`, 5 < K <= 128): shared by tests/test_gpu_stream_bonus.py,
which runs them on the device, and tests/test_stream_bonus_inputs.py, which checks on the host that they reach the states
they are here for (tests/bonus_restate.py)."""
import os

import numpy as np

from test_gpu_subtree_step import SHAPES          # (odd sequence's length, the others' length): windows of 1 - 64 rows, 1 - 3 columns
from util import GOLDEN

BOUNDARY_K = [6, 10, 11, 21, 33]                    # the votes go five anchors per sweep
BOUNDARY_SEED = {6: 506, 10: 510, 11: 611, 21: 821, 33: 533}      # (chosen so that rows with more than five entries are many)


def scoring(dna):
    z = np.load(os.path.join(GOLDEN, "param_tables.npz"))
    return (z["subm_1_0"], z["scal_1_0"].copy()) if dna else (z["subm_0_3"], z["scal_0_3"].copy())


def pairs_then_random_tree(n, rng):
    """every sequence first meets another sequence (n / 2 seq-seq tasks), then a random tree over the pairs"""
    tasks, nodes, nxt = [], [], n
    order = rng.permutation(n)
    for q in range(0, n - 1, 2):
        tasks.append((int(order[q]), int(order[q + 1]), nxt)); nodes.append(nxt); nxt += 1
    if n & 1:
        nodes.append(int(order[-1]))
    while len(nodes) > 1:
        i, j = rng.choice(len(nodes), 2, replace=False)
        tasks.append((nodes[i], nodes[j], nxt))
        nodes = [x for q, x in enumerate(nodes) if q not in (i, j)] + [nxt]
        nxt += 1
    return np.array(tasks, np.int32)


def noisy_family(rng, n, lo, hi, alpha, sub=0.3, indel=0.08):
    """n sequences of lo .. hi letters from one root: substitutions, short indels, ragged ends -- divergent enough that the
    anchors' pairwise alignments disagree about which residues belong together"""
    root = rng.randint(0, alpha, hi + 16).astype(np.uint8)
    out = []
    for _ in range(n):
        s = root[rng.randint(0, 6):].copy()
        m = rng.rand(len(s)) < sub
        s[m] = rng.randint(0, alpha, int(m.sum()))
        for _ in range(rng.poisson(indel * len(s))):
            p = rng.randint(0, len(s))
            k = 1 + rng.randint(0, 3)
            if rng.rand() < 0.5 and len(s) > 4 * k:
                s = np.concatenate([s[:p], s[p + k:]])
            else:
                s = np.concatenate([s[:p], rng.randint(0, alpha, k).astype(np.uint8), s[p:]])
        L = rng.randint(lo, hi + 1)
        out.append(np.ascontiguousarray(s[:L]))
    return out


def boundary_job(k):
    """24 - 40 short noisy sequences, nucleotides for odd K; K anchors"""
    rng = np.random.RandomState(BOUNDARY_SEED[k])
    dna = bool(k & 1)
    n = max(k + 3, 24 + (7 * k) % 17)
    codes = noisy_family(rng, n, 12, 65, 4 if dna else 20)
    return codes, pairs_then_random_tree(n, rng), rng.uniform(0.2, 1.2, n).astype(np.float32), dna


def k128_job(dna):
    """130 sequences of 24 - 40 letters: every anchor slot of the kernels in use"""
    rng = np.random.RandomState(900 + int(dna))
    codes = noisy_family(rng, 130, 24, 40, 4 if dna else 20)
    return codes, pairs_then_random_tree(130, rng), rng.uniform(0.2, 1.2, 130).astype(np.float32), dna


def shape_job(la, lb, dna):
    """8 related sequences, the first la letters long, the rest around lb.  The tree puts the odd one into a seq-seq task, its
    profile into a seq-profile task and that into a profile-profile task; the rest give seq-seq, profile-profile and
    seq-profile tasks among sequences of about lb letters."""
    rng = np.random.RandomState(17 * la + lb + (3000 if dna else 0))
    alpha = 4 if dna else 20
    base = rng.randint(0, alpha, max(la, lb) + 8).astype(np.uint8)
    codes = [np.ascontiguousarray(base[:la])]
    for q in range(1, 8):
        L = lb if q == 1 else max(1, lb + rng.randint(-2, 3))
        o = 0 if q == 1 else rng.randint(0, 4)         # shifted starts: the anchors disagree, rows carry several entries
        s = base[o:o + L].copy()
        m = rng.rand(L) < 0.3
        s[m] = rng.randint(0, alpha, int(m.sum()))
        if L > 4 and rng.rand() < 0.5:
            p = rng.randint(1, L - 2)
            s = np.concatenate([s[:p], s[p + 2:]])
        codes.append(np.ascontiguousarray(s))
    tasks = np.array([(0, 1, 8), (8, 2, 9), (3, 4, 10), (5, 6, 11), (10, 11, 12), (9, 12, 13), (13, 7, 14)], np.int32)
    return codes, tasks, np.linspace(0.2, 1.1, 8).astype(np.float32), dna


def refine_job():
    """a small noisy protein family for the refinement modes at K = 11"""
    rng = np.random.RandomState(77)
    codes = noisy_family(rng, 14, 30, 70, 20)
    return codes, pairs_then_random_tree(14, rng), rng.uniform(0.2, 1.2, 14).astype(np.float32), False
