"""GPU: KALIGN_REFINE_CONFIDENT for a batch of families (Context.run_families(refine=2), ka_run_encoded_batch): every family is
refined by the median confidence of its OWN edges, so it comes out as run_encoded(refine=2) aligns it alone -- the path
tests/test_gpu_run_encoded.py pins to the reference.  Rows byte for byte, thresholds as bits.  The families of a job differ in
divergence, and the test asserts from the families' own confidences that a median pooled over a job would mark other edges."""
import numpy as np
import pytest

from util import Golden

pytestmark = pytest.mark.gpu

# (sequences, residues, seed, substitution rate): sizes 3 and 4 fall below five anchors, 2 gets no table, 16 / 17 sit at the distance
# tile's edge; close and distant families alternate, so the medians of one job's families lie far apart
FAMILIES = [(1, 50, 700, 0.12), (2, 60, 701, 0.40), (3, 80, 702, 0.03), (4, 90, 703, 0.40), (5, 100, 704, 0.03),
            (16, 120, 705, 0.40), (17, 130, 706, 0.03), (40, 110, 707, 0.40), (2, 40, 708, 0.03), (3, 70, 709, 0.40), (4, 50, 710, 0.03)]
VARIANTS = {"fast": dict(n_anchors=0), "cons": dict(n_anchors=5), "cons_realign": dict(n_anchors=5, realign=1)}
JOBS = {"fast": 1, "cons": 4, "cons_realign": 4}                 # anchor counts 0 | 0 (two sequences), 3, 4, 5


@pytest.fixture(scope="module")
def ctx():
    import kalign_amd
    c = kalign_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scoring():
    g = Golden("tree_prot32x200")
    return g.subm, g.scal


@pytest.fixture(scope="module")
def families():
    from kalign_amd import guide, synth
    fams = [synth.family(n, length, seed=seed, sub_rate=sub) for n, length, seed, sub in FAMILIES]
    fams.append([synth.family(1, 70, seed=720)[0]] * 8)          # identical sequences: several edges tie exactly at the median
    return [(guide.encode_tree(s), guide.encode(s), s) for s in fams]


def median32(v):
    v = np.sort(np.asarray(v, np.float32))
    n = len(v)
    return v[n // 2] if n % 2 else np.float32(np.float32(v[n // 2 - 1] + v[n // 2]) / np.float32(2.0))


@pytest.fixture(scope="module")
def alone(ctx, families, scoring):
    """per variant and refinement mode, computed once and left unchanged: every family alone through run_encoded -- its rows, and
    the exact first-pass confidences of its final tree (the job run_encoded leaves on the context, run again depth first: mode 4)"""
    cache = {}

    def run(f, variant, refine):
        return ctx.run_encoded(f[0], f[1], f[2], scoring[0], scoring[1], weight=2.0, n_threads=2, refine=refine, **VARIANTS[variant])

    def get(variant, refine):
        if variant not in cache:
            confs = []
            for f in families:
                confs.append(np.zeros(0, np.float32))
                if len(f[1]) > 1:
                    run(f, variant, 0)
                    ctx.tree_refine(4)
                    confs[-1] = np.array([r.confidence for r in ctx.tree_download(want_gaps=False)[0]], np.float32)
            cache[variant] = confs
        if (variant, refine) not in cache:
            cache[(variant, refine)] = [[f[2][0].encode()] if len(f[1]) == 1 else run(f, variant, refine) for f in families]
        return cache[(variant, refine)], cache[variant]
    return get


def jobs_of(families, n_anchors):
    """the forest jobs of a batch: families of two sequences and more, by anchor count"""
    groups = {}
    for k, f in enumerate(families):
        n = len(f[1])
        if n >= 2:
            groups.setdefault(min(n_anchors, n) if n_anchors > 0 and n >= 3 else 0, []).append(k)
    return [groups[K] for K in sorted(groups)]


@pytest.mark.parametrize("refine", [2, 2 | 256], ids=["confident", "confident_adaptive"])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_batch_equals_every_family_alone(ctx, families, alone, scoring, variant, refine):
    want, confs = alone(variant, refine)
    got = ctx.run_families(families, scoring[0], scoring[1], weight=2.0, n_threads=2, refine=refine, **VARIANTS[variant])
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (variant, k, len(w))
    assert ctx.batch_stats()["jobs"] == JOBS[variant]
    assert len(set(got[-1])) == 1                                 # identical sequences: identical rows
    # ---- what the rule came to, per family ----
    st = ctx.batch_refine_stats(len(families))
    for k, (f, cf) in enumerate(zip(families, confs)):
        n = len(f[1])
        assert len(cf) == n - 1 and st["edges"][k] == n - 1
        thr = median32(cf) if n > 1 else np.float32(0.0)
        assert st["thr"][k].view(np.uint32) == thr.view(np.uint32), (variant, k, st["thr"][k], thr)
        assert st["refined"][k] == int((cf <= thr).sum())
        if n == 2:
            assert st["refined"][k] == 1                          # one edge: always refined
    # identical sequences: the edges between two sequences all have one confidence, and it is the family's median (an edge
    # with a profile on a side has four times the margin per member pair) -- a tie at the threshold, and every tied edge is refined
    tied = int((confs[-1] == st["thr"][-1]).sum())
    assert tied >= 2 and st["refined"][-1] == tied == int((confs[-1] <= st["thr"][-1]).sum())
    # ---- the batch shows something: in at least one job a median pooled over the job marks other edges ----
    differ = 0
    for job in jobs_of(families, VARIANTS[variant]["n_anchors"]):
        cj = np.concatenate([confs[k] for k in job])
        own = np.concatenate([confs[k] <= median32(confs[k]) for k in job])
        differ += int(((cj <= median32(cj)) != own).sum())
    assert differ >= 1
    assert len(jobs_of(families, VARIANTS[variant]["n_anchors"])) == JOBS[variant]


def test_stats_and_mode_errors(ctx, families, scoring):
    from kalign_amd import KalignAmdError
    import kalign_amd
    few = families[1:4]
    c = kalign_amd.Context(0)
    try:
        with pytest.raises(KalignAmdError, match="no finished ka_run_encoded_batch"):
            c.batch_refine_stats(3)
    finally:
        c.close()
    ctx.run_families(few, scoring[0], scoring[1], refine=2)
    assert list(ctx.batch_refine_stats(3)["edges"]) == [1, 2, 3]
    with pytest.raises(KalignAmdError, match="n_fam is not the last batch's"):
        ctx.batch_refine_stats(4)
    ctx.run_families(few, scoring[0], scoring[1], refine=1)
    with pytest.raises(KalignAmdError, match="did not run refine_mode 2"):
        ctx.batch_refine_stats(3)
    with pytest.raises(KalignAmdError, match="refine_mode must be 0, 1, 2"):
        ctx.run_families(few, scoring[0], scoring[1], refine=2 | 256 | 1 << 16)
    with pytest.raises(KalignAmdError, match="refine_mode must be"):
        ctx.run_families(few, scoring[0], scoring[1], refine=3 | 256)
