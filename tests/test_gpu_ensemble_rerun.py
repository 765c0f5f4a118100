"""GPU: ensemble.rerun_refined_batch -- the refinement re-runs finish_ensembles asks for (the selected members again with
KALIGN_REFINE_CONFIDENT, ensemble.c:403-451) as one Context.run_families(refine=2) per distinct member instead of one
run_encoded(refine=2) per family.  Rows against run_encoded on every family alone, byte for byte."""
import numpy as np
import pytest

from util import Golden

pytestmark = pytest.mark.gpu

SIZES = [(8, 60, 810), (12, 64, 811), (10, 56, 812)]
GAP_SCALE = [1.0, 0.75, 1.4]                                     # a member's gap penalties, as kalign_ensemble scales them per member
ASK = [(0, 1), (1, 0), (2, 1)]
RUN_KW = dict(n_anchors=5, weight=2.0, n_threads=2)


@pytest.fixture(scope="module")
def ctx():
    import kalign_amd
    c = kalign_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def setup():
    from kalign_amd import guide, synth
    g = Golden("tree_prot32x200")
    fams = []
    for n, length, seed in SIZES:
        s = synth.family(n, length, seed=seed, sub_rate=0.25)
        fams.append((guide.encode_tree(s), guide.encode(s), s))
    rng = np.random.RandomState(77)
    # member 0 has the plain tree; the others a block of n * min(32, n) multipliers >= 0.1 per family
    noise = {(k, f): np.maximum(0.1, rng.normal(1.0, 0.3, n * min(32, n))).astype(np.float32)
             for k in (1, 2) for f, (n, _, _) in enumerate(SIZES)}

    def member(k, fs):
        scal = np.array(g.scal, np.float32)
        scal[:3] *= np.float32(GAP_SCALE[k])
        return scal, (None if k == 0 else [noise[(k, f)] for f in fs])
    return g.subm, fams, member


class Counting:
    """a context that counts the batch calls made through it"""

    def __init__(self, ctx):
        self.ctx, self.calls = ctx, []

    def run_families(self, families, *a, **kw):
        self.calls.append(len(families))
        return self.ctx.run_families(families, *a, **kw)


@pytest.fixture(scope="module")
def alone(ctx, setup):
    subm, fams, member = setup
    out = []
    for f, k in ASK:
        scal, dms = member(k, [f])
        out.append(ctx.run_encoded(fams[f][0], fams[f][1], fams[f][2], subm, scal, dm_scale=None if dms is None else dms[0], refine=2, **RUN_KW))
    return out


def test_rows_equal_run_encoded_in_one_call_per_member(ctx, setup, alone):
    from kalign_amd import ensemble
    subm, fams, member = setup
    counting = Counting(ctx)
    asked = []

    def watched(k, fs):
        asked.append((k, list(fs)))
        return member(k, fs)
    got = ensemble.rerun_refined_batch(counting, fams, subm, watched, **RUN_KW)(ASK)
    assert got == alone
    assert counting.calls == [1, 2] and asked == [(0, [1]), (1, [0, 2])]       # one batch call per distinct member
    # the members differ: member 1's parameters give family 0 other rows than member 0's
    scal0, _ = member(0, [0])
    assert ctx.run_encoded(fams[0][0], fams[0][1], fams[0][2], subm, scal0, refine=2, **RUN_KW) != alone[0]


def test_ranks_put_rows_back_into_input_order(ctx, setup, alone):
    from kalign_amd import ensemble
    subm, fams, member = setup
    rng = np.random.RandomState(5)
    ranks = [rng.permutation(len(f[1])) for f in fams]
    got = ensemble.rerun_refined_batch(ctx, fams, subm, member, ranks=ranks, **RUN_KW)(ASK)
    for (f, _), rows, want in zip(ASK, got, alone):
        assert sorted(rows) == sorted(want)
        for i, r in enumerate(ranks[f]):
            assert rows[int(r)] == want[i]
    # the callable is what finish_ensembles takes: a list of (family, member) in, as many alignments out, in that order
    assert ensemble.rerun_refined_batch(ctx, fams, subm, member, **RUN_KW)([(2, 1)]) == [alone[2]]
