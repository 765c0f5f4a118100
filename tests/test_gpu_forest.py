"""Launches of the 4-wave kind (unit 2 of kalign_amd/csrc/ka_kernels.hip: two workgroups per CU).  A launch takes that kernel when
a guide-tree level has more tasks than the GPU has CUs: forests of the reference's goldens (every copy must come out as the golden
does: aln_seqseq.c / aln_seqprofile.c / aln_profileprofile.c through the Hirschberg recursion of aln_controller.c, bit for bit)."""
import numpy as np
import pytest

from util import Golden, compare_recs, tree_cases

pytestmark = pytest.mark.gpu

EXACT = ["len_a", "len_b", "nsip_a", "nsip_b", "plen", "kind", "swapped", "meet", "transition", "gap_scale", "subm_off", "score"]
# goldens whose scoring tables and penalties are the plain ones of the forest below (every copy shares one subm / scal)
COPIES = 40


@pytest.mark.parametrize("name", tree_cases())
def test_forest_of_goldens(name):
    """40 copies of a golden tree as one forest: the lower levels hold more tasks than CUs and go to the 4-wave kind of launch"""
    import kalign_amd
    from kalign_amd import guide
    g = Golden(name)
    if len(g.lens) < 8:
        pytest.skip("too few tasks per level even as a forest")
    sd = g.seq_distances
    # dependency levels of the tree; a level goes to the 4-wave kind of launch when it holds more tasks than the GPU has CUs
    # (256) and not only seq-seq ones -- enough copies that the widest mixed level of the forest does
    n, depth, mixed = len(g.lens), {}, {}
    for a, b, c in np.asarray(g.tasks):
        d = 1 + max(depth.get(int(a), 0), depth.get(int(b), 0))
        depth[int(c)] = d
        if a >= n or b >= n:
            mixed[d] = mixed.get(d, 0) + 1
    copies = max(COPIES, 300 // max(mixed.values()) + 1)
    fc, ft, fd, spans = guide.forest([(g.codes, g.tasks, sd)] * copies if sd is not None else [(g.codes, g.tasks)] * copies)
    ctx = kalign_amd.Context(0)
    try:
        recs, paths, gaps = ctx.msa_tree(fc, ft, g.subm, g.scal, fd)
        assert ctx.fallback_runs() == 0
        want_gaps = g.gaps_list()
        for (s0, t0, ns, nt) in spans:
            sub = recs[t0:t0 + nt]
            assert compare_recs(g, sub, paths, EXACT) == [], (name, t0)
            for got, want in zip(gaps[s0:s0 + ns], want_gaps):
                assert np.array_equal(got, want)
    finally:
        ctx.close()

