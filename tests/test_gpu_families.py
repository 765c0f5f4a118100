"""GPU: a batch of families from letters to rows in one call (ka_run_encoded_batch, Context.run_families), the guide
trees and realignment trees of a batch (ka_guide_forest, ka_aln_guide_forest) -- against the rows the real reference
produced (tests/golden) and against run_encoded on every family alone, which tests/test_gpu_run_encoded.py pins
against the reference.  Everything is compared byte for byte, floats as bits."""
import os

import numpy as np
import pytest

from util import GOLDEN, Golden, random_rows

pytestmark = pytest.mark.gpu

POISON = 16                                  # KA_DEBUG_POISON_ARENAS, as tests/test_gpu_poison.py sets it


@pytest.fixture(scope="module")
def ctx():
    import kalign_amd
    c = kalign_amd.Context(0)
    yield c
    c.close()


def input_order(ranks, rows):
    out = [None] * len(rows)
    for i, r in enumerate(ranks):
        out[int(r)] = rows[i].decode()
    return out


def golden_family(name):
    g = Golden(name)
    return g, (g.tree_seqs, g.codes, g.sorted_seqs())


def realign_family(name):
    from kalign_amd import guide
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    off = np.concatenate([[0], np.cumsum(z["lens"])])
    codes = [z["codes"][off[i]:off[i + 1]] for i in range(len(z["lens"]))]
    letters = [str(z["seqs"][r]) for r in z["ranks"]]
    return z, (guide.encode_tree(letters, dna=int(z["biotype"]) != 0), codes, letters)


def check_goldens(ctx, names, **kw):
    gs, fams = zip(*[golden_family(n) for n in names])
    for g in gs[1:]:                                              # one batch shares its scoring
        assert np.array_equal(g.subm, gs[0].subm) and np.array_equal(g.scal, gs[0].scal)
    rows = ctx.run_families(list(fams), gs[0].subm, gs[0].scal, n_threads=2, **kw)
    assert len(rows) == len(names)
    for name, g, r in zip(names, gs, rows):
        assert input_order(g.ranks, r) == [str(x) for x in g.rows], name


def test_fast_mode_protein(ctx):
    check_goldens(ctx, ["tree_BB11001", "tree_BB12006", "tree_BB30014", "tree_prot32x200", "tree_ragged"])


def test_fast_mode_nucleotides(ctx):
    check_goldens(ctx, ["tree_dna4", "tree_rna16x300"])


def test_default_mode_with_a_family_below_the_anchor_count(ctx):
    """cons_BB11001 has 4 sequences and gets 4 anchors, the others 5: two forest jobs behind one call"""
    names = ["cons_BB11001", "cons_BB30014", "cons_prot32x200", "cons_ragged"]
    for n in names:
        g = Golden(n)
        assert int(g.n_anchors) == 5 and float(g.weight) == 2.0
    check_goldens(ctx, names, n_anchors=5, weight=2.0)
    assert ctx.batch_stats()["jobs"] == 2


def test_realignment(ctx):
    names = ["realign_dups", "realign_prot150", "realign_prot40"]
    zs, fams = zip(*[realign_family(n) for n in names])
    for z in zs:
        assert int(z["n_anchors"]) == int(zs[0]["n_anchors"]) and np.array_equal(z["scal"], zs[0]["scal"]) and np.array_equal(z["subm"], zs[0]["subm"])
    rows = ctx.run_families(list(fams), zs[0]["subm"], zs[0]["scal"], n_anchors=int(zs[0]["n_anchors"]), weight=float(zs[0]["weight"]), realign=1)
    for name, z, r in zip(names, zs, rows):
        assert input_order(z["ranks"], r) == [str(x) for x in z["final_rows"]], name


# ---- edges, against run_encoded on every family alone ----
EDGE_SIZES = [(1, 30), (2, 40), (3, 60), (16, 120), (17, 130), (49, 50), (50, 50), (51, 50), (520, 30)]
VARIANTS = {"fast_realign": dict(n_anchors=0, realign=1), "cons_realign": dict(n_anchors=5, realign=1),
            "refine1": dict(n_anchors=5, refine=1), "refine3": dict(n_anchors=5, refine=3)}


def as_family(seqs):
    from kalign_amd import guide
    return (guide.encode_tree(seqs), guide.encode(seqs), seqs)


@pytest.fixture(scope="module")
def edge_families():
    """family sizes at the distance tile's edge (16 / 17), around the bisection threshold (49, 50, 51), the first with two
    rows per UPGMA thread (520), the smallest (1, 2, 3); 16 x 120 and 17 x 130 without indels: alignments at most 128
    columns wide and just over (the 128-column staging step); one family of identical sequences"""
    from kalign_amd import synth
    fams = []
    for k, (n, length) in enumerate(EDGE_SIZES):
        fams.append(as_family(synth.family(n, length, seed=200 + k, indel_rate=0.0 if n in (16, 17) else 0.02)))
    fams.append(as_family([synth.family(1, 70, seed=300)[0]] * 8))
    return fams


@pytest.fixture(scope="module")
def scoring():
    g = Golden("tree_prot32x200")
    return g.subm, g.scal


@pytest.fixture(scope="module")
def edge_alone(ctx, edge_families, scoring):
    """run_encoded on every family alone, per variant, computed when first asked for and then left unchanged"""
    cache = {}

    def get(variant):
        if variant not in cache:
            kw = VARIANTS[variant]
            cache[variant] = [[bytes(f[2][0].encode())] if len(f[1]) == 1 else
                              ctx.run_encoded(f[0], f[1], f[2], scoring[0], scoring[1], weight=2.0, n_threads=2, **kw) for f in edge_families]
        return cache[variant]
    return get


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_edges_against_every_family_alone(ctx, edge_families, edge_alone, scoring, variant):
    want = edge_alone(variant)
    got = ctx.run_families(edge_families, scoring[0], scoring[1], weight=2.0, n_threads=2, **VARIANTS[variant])
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (variant, k, len(w))
    widths = [len(r[0]) for r in got]
    assert widths[3] <= 128 < widths[4] <= 256                  # the 16 x 120 and the 17 x 130 family
    assert len(set(got[-1])) == 1                                 # identical sequences: identical rows


def test_edges_on_poisoned_arenas(edge_families, edge_alone, scoring):
    import kalign_amd
    want = edge_alone("fast_realign")
    c = kalign_amd.Context(0)
    try:
        c.debug_set_hooks(POISON)
        got = c.run_families(edge_families, scoring[0], scoring[1], weight=2.0, n_threads=2, **VARIANTS["fast_realign"])
        assert c.fallback_runs() == 0
    finally:
        c.close()
    assert got == want


# ---- the trees of a batch on their own ----
def test_guide_forest_on_the_device(ctx):
    """two distance batches for all families: every family's tree is the one ka_guide_tree builds for it alone"""
    from kalign_amd import guide
    names = ["tree_BB30014", "tree_prot32x200", "tree_ragged"]
    gs = [Golden(n) for n in names]
    tasks, sd = ctx.guide_forest([g.tree_seqs for g in gs], n_threads=2)
    _, want, _, _ = guide.forest([(g.tree_seqs, g.tasks) for g in gs])
    assert np.array_equal(tasks, want)
    assert np.array_equal(sd.view(np.uint32), np.concatenate([g.seq_distances for g in gs]).view(np.uint32))


def check_forest_against_the_oracle(oracle, rows_of, tasks, sd, dms):
    """every family of a batch against oracle.aln_guide_tree of its own rows: distances and means as bits, the tasks in
    the forest's numbering.  A family of one row has no pair and no merge: distance 0 to itself, mean 0, no task."""
    from kalign_amd import guide
    lone = (np.zeros((0, 3), np.int32), np.zeros(1, np.float32), np.zeros((1, 1), np.float32))
    want = [oracle.aln_guide_tree(r) if len(r) > 1 else lone for r in rows_of]
    _, wtasks, _, _ = guide.forest([(r, w[0]) for r, w in zip(rows_of, want)])
    assert np.array_equal(tasks, wtasks.reshape(-1, 3))
    assert np.array_equal(sd.view(np.uint32), np.concatenate([w[1] for w in want]).view(np.uint32))
    assert len(dms) == len(want)
    for dm, w in zip(dms, want):
        assert np.array_equal(dm.view(np.uint32), w[2].view(np.uint32))


def test_aln_guide_forest(ctx, oracle):
    from kalign_amd import api, guide
    names = ["realign_dups", "realign_prot150", "realign_prot40"]
    zs, fams = zip(*[realign_family(n) for n in names])
    given = [[str(r).encode() for r in z["rows_sorted"]] for z in zs]
    assert len(set(len(f[0]) for f in given)) == 3                # three different widths

    def check(rows_of, tasks, sd, dms):
        alone = [ctx.aln_guide_tree(r, want_dm=True) for r in rows_of]
        _, want, _, _ = guide.forest([(r, a[0]) for r, a in zip(rows_of, alone)])
        assert np.array_equal(tasks, want)
        assert np.array_equal(sd.view(np.uint32), np.concatenate([a[1] for a in alone]).view(np.uint32))
        for dm, a in zip(dms, alone):
            assert np.array_equal(dm.view(np.uint32), a[2].view(np.uint32))
        check_forest_against_the_oracle(oracle, rows_of, tasks, sd, dms)
        return alone

    # rows from the host
    tasks, sd, dms = ctx.aln_guide_forest(given, want_dm=True)
    alone = check(given, tasks, sd, dms)
    for z, a in zip(zs, alone):                                   # ... which are the reference's
        assert np.array_equal(a[0], z["tasks2"]) and np.array_equal(a[2].view(np.uint32), z["dm"].view(np.uint32))
    # the rows a forest's tree_aligned_rows left in HBM
    codes, ftasks, fsd, spans = guide.forest([(f[1], z["tasks1"], z["seq_distances1"]) for z, f in zip(zs, fams)])
    ctx.tree_upload(codes, ftasks, zs[0]["subm"], zs[0]["scal"], fsd, flags=api.FLAG_DEVICE_GAPS)
    ctx.tree_run()
    rows = ctx.tree_aligned_rows([x for f in fams for x in f[2]])
    sizes = [s[2] for s in spans]
    per_family = [rows[s[0]:s[0] + s[2]] for s in spans]
    for z, r in zip(zs, per_family):
        assert [x.decode() for x in r] == [str(x) for x in z["rows_sorted"]]
    got = ctx.aln_guide_forest(None, sizes=sizes, want_dm=True)   # (before anything else touches the rows)
    check(per_family, *got)
    # distinct widths under one stride, a one-row family, the tile's and the staging step's edges inside a table
    edges = [random_rows(n, w, seed) for n, w, seed in ((1, 30, 21), (2, 1, 16), (16, 128, 22), (17, 129, 23), (520, 30, 24))]
    assert all(set(r) != {45} for f in edges for r in f)           # no row is all gaps
    check_forest_against_the_oracle(oracle, edges, *ctx.aln_guide_forest(edges, want_dm=True))


def test_family_above_the_one_workgroup_limit(ctx, scoring):
    """6200 sequences: more than the one-workgroup UPGMA takes (6144), so that family's merges run as per-merge launches
    beside the small families' workgroups"""
    from kalign_amd import synth
    fams = [as_family(synth.family(6200, 12, seed=400)), as_family(synth.family(20, 40, seed=401)), as_family(synth.family(5, 40, seed=402))]
    got = ctx.run_families(fams, scoring[0], scoring[1], realign=1, n_threads=4)
    for k, f in enumerate(fams):
        assert got[k] == ctx.run_encoded(f[0], f[1], f[2], scoring[0], scoring[1], realign=1, n_threads=4), k


def test_handing_over_the_rows(ctx):
    import kalign_amd
    from kalign_amd import api
    ga, fa = golden_family("tree_ragged")
    gb, fb = golden_family("tree_BB11001")
    first = ctx.run_families([fa, fb], ga.subm, ga.scal)
    need = int(ctx.L.ka_batch_rows_size(ctx.h))
    assert need == sum(len(f) * (len(f[0]) + 1) for f in first)  # packed: every family at its own width
    buf = np.full(need, 7, np.uint8)
    assert ctx.L.ka_batch_rows(ctx.h, api._ptr(buf), need - 1) != 0 and b"cap_bytes is smaller" in ctx.L.ka_last_error()
    assert (buf == 7).all()
    assert ctx.L.ka_batch_rows(ctx.h, api._ptr(buf), need) == 0   # nothing was lost
    w = len(first[0][0])
    assert buf[:w].tobytes() == first[0][0] and buf[w] == 0
    # a second batch replaces the first
    second = ctx.run_families([fb], ga.subm, ga.scal)
    assert int(ctx.L.ka_batch_rows_size(ctx.h)) == len(second[0]) * (len(second[0][0]) + 1)
    assert second[0] == first[1]
    # ka_aln_guide_tree knows one alignment only, as before
    ctx._job = dict(lens=None, ntasks=0, n=len(fb[1]))
    with pytest.raises(kalign_amd.KalignAmdError, match="no rows on the device"):
        ctx.aln_guide_tree()
    ctx.run_families([fa, fb], ga.subm, ga.scal, realign=1)
    ctx._job = dict(lens=None, ntasks=0, n=len(fa[1]) + len(fb[1]))
    with pytest.raises(kalign_amd.KalignAmdError, match="no rows on the device"):
        ctx.aln_guide_tree()
