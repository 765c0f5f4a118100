"""CPU: the marks of a KALIGN_REFINE_CONFIDENT pass (kalign_amd/csrc/ka_marks.cpp) without a GPU.  ka_debug_refine_marks hands out
what ka_tree_refine (one median pooled over the job) and ka_tree_refine_trees (a median per tree) compute before they launch: the
tree of every task, every tree's threshold and the marked tasks -- here against a numpy restatement of the rule, all in fp32:
a tree is the set of tasks that lead to one root (a task nobody consumes), trees are numbered by ascending root task, a tree of n
tasks has the threshold v[n/2] (n odd) or (v[n/2-1] + v[n/2]) / 2.0F (n even) of its sorted confidences
(compute_confidence_threshold, aln_refine.c:674-712), and a task is marked when its confidence is <= its tree's threshold."""
import numpy as np
import pytest

from util import Golden, refine_cases


def test_names_and_abi_version():
    import kalign_amd
    from kalign_amd import api, ensemble
    L = kalign_amd.load_library()
    for name in ("ka_debug_refine_marks", "ka_tree_refine_trees", "ka_batch_refine_stats"):
        assert name in api.EXPORTS and hasattr(L, name)
    assert L.ka_abi_version() >= 22
    assert callable(api.Context.tree_refine_trees) and callable(api.Context.batch_refine_stats) and callable(ensemble.rerun_refined_batch)


def marks(numseq, tasks, conf, pooled=False):
    from kalign_amd import api
    return api.refine_marks(numseq, tasks, conf, pooled=pooled)


def median32(v):
    v = np.sort(np.asarray(v, np.float32))
    n = len(v)
    return v[n // 2] if n % 2 else np.float32(np.float32(v[n // 2 - 1] + v[n // 2]) / np.float32(2.0))


def restate(numseq, tasks, conf, pooled=False):
    tasks = np.asarray(tasks).reshape(-1, 3)
    conf = np.asarray(conf, np.float32)
    nt = len(tasks)
    maker, parent = {}, [-1] * nt
    for t, (a, b, c) in enumerate(tasks):
        maker[int(c)] = t
        for ch in (int(a), int(b)):
            if ch >= numseq:
                parent[maker[ch]] = t
    roots = [t for t in range(nt) if parent[t] < 0]
    tree_of = np.zeros(nt, np.int32)
    for t in range(nt):
        r = t
        while parent[r] >= 0:
            r = parent[r]
        tree_of[t] = roots.index(r)
    if pooled:
        thr = np.full(len(roots), median32(conf), np.float32)
    else:
        thr = np.array([median32(conf[tree_of == k]) for k in range(len(roots))], np.float32)
    return tree_of, thr, (conf <= thr[tree_of]).astype(np.int32)


def check(numseq, tasks, conf, pooled=False):
    got = marks(numseq, tasks, conf, pooled)
    want = restate(numseq, tasks, conf, pooled)
    assert np.array_equal(got[0], want[0])
    assert got[1].dtype == np.float32 and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    assert np.array_equal(got[2], want[2])
    return got


def tree(n, seed):
    from kalign_amd import guide
    return guide.bisecting_tree(n, seed=seed)


def forest(sizes, seed=0):
    """trees of the given numbers of leaves one after the other: (numseq, tasks)"""
    from kalign_amd import guide
    _, tasks, _, _ = guide.forest([(list(range(n)), tree(n, seed + k)) for k, n in enumerate(sizes)])
    return sum(sizes), tasks


def confidences(n, seed):
    """distinct float32 values whose pairwise means are not all representable exactly: the fp32 rounding of the even rule shows"""
    rng = np.random.RandomState(seed)
    return (rng.random_sample(n) * 100.0).astype(np.float32)


@pytest.mark.parametrize("leaves", [8, 9, 2, 3, 32, 44])
def test_one_tree(leaves):
    """odd and even numbers of tasks (7, 8, 31, 43), a tree of one task and one of two"""
    tasks = tree(leaves, 3)
    conf = confidences(leaves - 1, leaves)
    tree_of, thr, m = check(leaves, tasks, conf)
    assert not tree_of.any() and len(thr) == 1
    assert thr[0] == median32(conf)
    assert np.array_equal(np.array([thr[0]]).view(np.uint32), np.array([np.median(conf)], np.float32).view(np.uint32))
    assert int(m.sum()) == (leaves - 1 + 1) // 2          # distinct values: the lower half, with the middle one for odd n
    # one tree: pooled and per tree are one rule
    for a, b in zip(check(leaves, tasks, conf, pooled=True), (tree_of, thr, m)):
        assert np.array_equal(a, b)


def test_a_tree_of_one_task_is_always_marked():
    numseq, tasks = forest([2, 2, 5])
    conf = np.array([99.0, 1.0, 5.0, 6.0, 7.0, 8.0], np.float32)
    tree_of, thr, m = check(numseq, tasks, conf)
    assert list(tree_of) == [0, 1, 2, 2, 2, 2] and list(thr) == [99.0, 1.0, 6.5] and list(m) == [1, 1, 1, 1, 0, 0]
    # pooled, the high single edge is not refined: the rule ka_tree_refine keeps on a forest
    _, pthr, pm = check(numseq, tasks, conf, pooled=True)
    assert list(pthr) == [6.5] * 3 and list(pm) == [0, 1, 1, 1, 0, 0]


def test_three_trees_one_after_the_other():
    sizes = [7, 4, 6]                                      # 6, 3 and 5 tasks
    numseq, tasks = forest(sizes, seed=10)
    # the middle tree's confidences lie far above the others': per tree half of each is marked, pooled none of it
    conf = np.concatenate([confidences(6, 1), confidences(3, 2) + np.float32(200.0), confidences(5, 3)])
    tree_of, thr, m = check(numseq, tasks, conf)
    assert list(tree_of) == [0] * 6 + [1] * 3 + [2] * 5 and len(thr) == 3
    assert [int(m[tree_of == k].sum()) for k in range(3)] == [3, 2, 3]
    ptree_of, pthr, pm = check(numseq, tasks, conf, pooled=True)
    assert np.array_equal(ptree_of, tree_of) and len(set(pthr.tolist())) == 1 and pthr[0] == median32(conf)
    assert int(pm[tree_of == 1].sum()) == 0 and not np.array_equal(pm, m)


def test_interleaved_trees_are_numbered_by_their_roots():
    """the same three trees with their tasks dealt round-robin, children still before parents: the smallest tree's root comes
    first, so it is tree 0, and every tree keeps the threshold of its own confidences"""
    sizes = [7, 4, 6]
    numseq, tasks = forest(sizes, seed=10)
    conf = np.concatenate([confidences(6, 1), confidences(3, 2) + np.float32(200.0), confidences(5, 3)])
    _, thr_seq, m_seq = marks(numseq, tasks, conf)
    first = np.concatenate([[0], np.cumsum([n - 1 for n in sizes])])
    order = []
    for k in range(max(sizes)):
        order += [int(first[j]) + k for j in range(3) if k < sizes[j] - 1]
    order = np.array(order)
    assert sorted(order.tolist()) == list(range(len(tasks))) and order.tolist() != sorted(order.tolist())
    tree_of, thr, m = check(numseq, tasks[order], conf[order])
    roots_at = {int(np.nonzero(order == first[j + 1] - 1)[0][0]): j for j in range(3)}     # position of every tree's root -> tree
    number = {roots_at[p]: i for i, p in enumerate(sorted(roots_at))}                       # sequential tree -> its number now
    assert number == {1: 0, 2: 1, 0: 2}
    for pos, t in enumerate(order):
        j = int(np.searchsorted(first, t, side="right")) - 1
        assert tree_of[pos] == number[j]
        assert m[pos] == m_seq[t]
    for j in range(3):
        assert thr[number[j]].view(np.uint32) == thr_seq[j].view(np.uint32)


def test_ties_at_the_median_are_all_marked():
    numseq, tasks = forest([6, 5, 4])
    conf = np.array([1, 2, 2, 2, 3,    4, 4, 4, 4,    5, 7, 7], np.float32)
    tree_of, thr, m = check(numseq, tasks, conf)
    assert list(thr) == [2.0, 4.0, 7.0]
    assert list(m) == [1, 1, 1, 1, 0,    1, 1, 1, 1,    1, 1, 1]
    # identical sequences: every edge has the same confidence, every edge ties at the median, every edge is refined
    _, thr1, m1 = check(numseq, tasks, np.full(12, 3.25, np.float32))
    assert list(thr1) == [3.25] * 3 and m1.all()


@pytest.mark.parametrize("name", [n for n in refine_cases() if "_conf" in n])
def test_goldens_threshold_is_the_median_of_conf_before(name):
    g = Golden(name)
    conf = np.asarray(g.conf_before, np.float32)
    tree_of, thr, m = check(len(g.lens), g.tasks, conf)
    med = np.median(conf)
    assert med.dtype == np.float32
    assert len(thr) == 1 and thr[0].view(np.uint32) == med.view(np.uint32)
    assert np.array_equal(m, (conf <= med).astype(np.int32))


def test_bad_input_is_refused_with_its_cause():
    from kalign_amd import KalignAmdError
    conf3 = np.ones(3, np.float32)
    with pytest.raises(KalignAmdError, match="task 1.*consumed twice"):
        marks(4, [(0, 1, 4), (4, 4, 5), (2, 3, 6)], conf3)                 # both operands of one task
    with pytest.raises(KalignAmdError, match="task 2.*consumed twice"):
        marks(5, [(0, 1, 5), (5, 2, 6), (5, 3, 7)], conf3)                 # node 5 feeds two tasks
    with pytest.raises(KalignAmdError, match="task 0.*children before parents"):
        marks(4, [(0, 5, 4), (1, 2, 5), (4, 3, 6)], conf3)                 # a child index not below its parent's: node 5 is made later
    with pytest.raises(KalignAmdError, match="children before parents"):
        marks(4, [(0, 1, 4), (2, 3, 4), (4, 3, 6)], conf3)                 # node 4 made twice
    with pytest.raises(KalignAmdError, match="children before parents"):
        marks(4, [(0, 1, 3), (2, 3, 5), (4, 5, 6)], conf3)                 # a task that makes a sequence
    with pytest.raises(KalignAmdError, match="n_tasks"):
        marks(3, [(0, 1, 3), (3, 2, 4), (0, 1, 5)], conf3)                 # more tasks than merges
    with pytest.raises(KalignAmdError, match="one confidence per task"):
        marks(4, [(0, 1, 4), (2, 3, 5)], conf3)
