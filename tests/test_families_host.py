"""The guide trees of a batch of families (ka_guide_forest_from): the three phases of build_tree_kmeans run over all
families before the next starts, so the distance source is called at most twice -- and every family's tasks and
seq_distances are, bit for bit, what ka_guide_tree_from gives that family alone.  CPU only: the distances come from the
oracle's bpm_block restatement, as in tests/test_guide_tree.py."""
import numpy as np
import pytest

from util import Golden

GOLDENS = ["tree_BB11001", "tree_BB12006", "tree_BB30014", "tree_prot32x200", "tree_ragged"]


def test_names_and_version():
    import kalign_amd
    from kalign_amd import api
    L = kalign_amd.load_library()
    for name in ("ka_guide_forest_from", "ka_guide_forest", "ka_aln_guide_forest", "ka_run_encoded_batch", "ka_batch_rows_size", "ka_batch_rows"):
        assert name in api.EXPORTS and hasattr(L, name), name
    assert L.ka_abi_version() >= 17
    for name in ("run_families", "guide_forest", "aln_guide_forest"):
        assert hasattr(kalign_amd.Context, name), name
    assert callable(api.guide_forest_from)


@pytest.fixture(scope="module")
def families():
    """per family the sequences in the tree alphabet: five goldens, 140 sequences (bisection above 50), two, one"""
    from kalign_amd import guide, synth
    fams = [Golden(name).tree_seqs for name in GOLDENS]
    big = sorted(synth.family(140, 60, seed=77), key=lambda s: -len(s))
    fams.append(guide.encode_tree(big))
    fams.append(guide.encode_tree(synth.family(2, 40, seed=78)))
    fams.append(guide.encode_tree(synth.family(1, 30, seed=79)))
    return fams


@pytest.fixture(scope="module")
def alone(oracle, families):
    """ka_guide_tree_from on every family alone (None for the family of one sequence), computed once"""
    from kalign_amd import api
    out = []
    for f in families:
        if len(f) < 2:
            out.append(None)
            continue
        out.append(api.guide_tree_from([len(s) for s in f], lambda ia, ib, f=f: oracle.bpm_batch(f, ia, ib)))
    return out


def expected_forest(families, alone):
    from kalign_amd import guide
    jobs = [(f, a[0] if a is not None else np.zeros((0, 3), np.int32)) for f, a in zip(families, alone)]
    _, tasks, _, _ = guide.forest(jobs)
    sd = np.concatenate([a[1] if a is not None else np.zeros(1, np.float32) for a in alone])
    return tasks.reshape(-1, 3), sd


@pytest.mark.parametrize("n_threads", [1, 4])
def test_forest_equals_the_single_family_builder(oracle, families, alone, n_threads):
    from kalign_amd import api
    seqs = [s for f in families for s in f]
    fam_of = np.concatenate([np.full(len(f), k) for k, f in enumerate(families)])
    calls = []

    def dist(ia, ib):
        calls.append(len(ia))
        assert np.array_equal(fam_of[ia], fam_of[ib])             # never a pair that spans two families
        return oracle.bpm_batch(seqs, ia, ib)

    tasks, sd = api.guide_forest_from([[len(s) for s in f] for f in families], dist, n_threads=n_threads)
    assert len(calls) <= 2
    want_tasks, want_sd = expected_forest(families, alone)
    assert np.array_equal(tasks, want_tasks)
    assert np.array_equal(sd.view(np.uint32), want_sd.view(np.uint32))
    # the golden families carry the reference's own trees
    for k, name in enumerate(GOLDENS):
        assert np.array_equal(alone[k][0], Golden(name).tasks)
    assert sd[sum(len(f) for f in families) - 1] == 0.0           # the family of one sequence


def test_noisy_form(oracle):
    """dm_scale blocks of two families: each family equals its guide_tree_from(..., dm_scale=block)"""
    from kalign_amd import api
    a, b = Golden("guide_noisy_prot40"), Golden("guide_noisy_dna200")
    seqs = list(a.tree_seqs) + list(b.tree_seqs)
    tasks, sd = api.guide_forest_from([a.lens, b.lens], lambda ia, ib: oracle.bpm_batch(seqs, ia, ib), n_threads=2,
                                      dm_scale=[a.dm_scale, b.dm_scale])
    alone = [api.guide_tree_from(g.lens, lambda ia, ib, g=g: oracle.bpm_batch(g.tree_seqs, ia, ib), dm_scale=g.dm_scale) for g in (a, b)]
    for g, one in zip((a, b), alone):                             # ... which is the reference's noisy tree
        assert np.array_equal(one[0], g.tasks)
    want_tasks, want_sd = expected_forest([a.tree_seqs, b.tree_seqs], alone)
    assert np.array_equal(tasks, want_tasks)
    assert np.array_equal(sd.view(np.uint32), want_sd.view(np.uint32))


def test_error_cases_are_named():
    import kalign_amd
    from kalign_amd import api
    zeros = lambda ia, ib: np.zeros(len(ia), np.int32)            # noqa: E731
    with pytest.raises(kalign_amd.KalignAmdError, match="empty family"):
        api.guide_forest_from([[5, 4, 3], [], [6, 2]], zeros)
    with pytest.raises(kalign_amd.KalignAmdError, match="zero-length sequence"):
        api.guide_forest_from([[5, 4, 3], [6, 0]], zeros)
    # fam_first itself: the wrapper always makes a good one, so straight through the C entry point
    L = kalign_amd.load_library()
    lens = np.array([5, 4, 3, 6, 2], np.int32)
    tasks = np.zeros((5, 3), np.int32)
    sd = np.zeros(5, np.float32)
    cb = api.DIST_FN(lambda user, n, ia, ib, out: 1)
    for first in ([1, 3, 5], [0, 4, 3]):
        ff = np.array(first, np.int32)
        rc = L.ka_guide_forest_from(2, api._ptr(ff), api._ptr(lens), cb, None, 1, None, api._ptr(tasks), None, api._ptr(sd))
        assert rc != 0 and b"fam_first does not ascend from 0 to numseq" in L.ka_last_error()
