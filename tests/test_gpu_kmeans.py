"""GPU: the 2-means bisection on the device (ka_kmeans.hip) pinned bit for bit, candidate by candidate.

A finished tree is blind to a rounding inside split2: a summation order, a contraction or a rounding that differs from
the reference's moves a few bits of a distance and leaves the tree as it was on almost every input.  So

* test_candidates_*: ONE level through ka_debug_kmeans_level -- the function the product's level loop calls -- and, for
  every candidate of every set, score, counts, both lists, every per-sample min(dl, dr) of the last iteration and the
  centroid against the host's split2 (ka_debug_kmeans_host), which tests/test_kmeans_split.py pins to the reference's
  real split2.  Inputs: tests/kmeans_cases.py;
* test_tree_*: whole matrices injected through the public ka_guide_tree (identical sequences of length 625: every
  distance is 0.0625 exactly, dm_scale = 16 * M makes the matrix M), device tree == host tree == (where its noise
  generator can produce the input) the real reference's tree.  All leaf-cluster distances tie, UPGMA takes the first
  pair every time, so the task list encodes every leaf cluster's membership and order.

What the candidate level sees and the trees do not: ka_kmeans.hip built once with -ffp-contract=fast and once with
km_edist's final combine as ((v0 + v1) + v2) + v3 passes all 32 test_tree_device_equals_host cases and fails 159 / 157 of
the 210 test_candidates_* cases, each at the min(dl, dr) assertion (scores differ in 83 / 91 of them, counts in 6 / 20,
the acceptance rule's winner in none).  split2's 500-iteration cap is reached by no input here (longest run 159) and
stays untested."""
import threading

import numpy as np
import pytest

import kmeans_cases as kc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import kalign_amd
    c = kalign_amd.Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _accept(score):
    """the reference's acceptance rule (bisectingKmeans.c:318-352) on one set's scores"""
    best = -1
    for i in range(0, len(score), 4):
        change = 0
        for c in range(i, min(i + 4, len(score))):
            if best < 0 or score[best] > score[c]:
                best, change = c, change + 1
        if not change:
            break
    return best


def _compare_level(ctx, kind, sizes, force_big):
    dm, samples, sets, host = kc.host_level(kind, sizes)
    dev, big = ctx.kmeans_level(dm, samples, sets, force_big=force_big)
    assert big == (force_big or max(sizes) > 1024)
    bad = dict(score=[], counts=[], lists=[], mind=[], wmean=[], winner=[])
    mind_elems = 0
    for k, (start, n) in enumerate(sets):
        d, hs = dev[k], host[k]
        if len(sizes) == 1:
            kc.check_conditions(kind, int(n), hs)
        assert len(d["score"]) == len(hs) == min(kc.TRIES, n)
        if not np.array_equal(_bits(d["wmean"]), _bits(hs[0]["wmean"])):
            bad["wmean"].append(k)
        for c, h in enumerate(hs):
            if _bits(d["score"][c]) != _bits(h["score"]):
                bad["score"].append((k, c))
            if tuple(d["counts"][c]) != tuple(h["counts"]):
                bad["counts"].append((k, c))
            elif not (np.array_equal(d["lists"][c, 0, :len(h["sl"])], h["sl"]) and np.array_equal(d["lists"][c, 1, :len(h["sr"])], h["sr"])):
                bad["lists"].append((k, c))
            diff = int(np.count_nonzero(_bits(d["mind"][c]) != _bits(h["mind"])))
            if diff:
                bad["mind"].append((k, c))
                mind_elems += diff
        if d["winner"] != _accept([h["score"] for h in hs]):
            bad["winner"].append(k)
    total = sum(len(h) for h in host)
    print("%s %s big=%d: of %d candidates differ in score %d, counts %d, lists %d, mind %d (%d elements); sets: wmean %d, winner %d"
          % (kind, sizes, big, total, len(bad["score"]), len(bad["counts"]), len(bad["lists"]), len(bad["mind"]), mind_elems,
             len(bad["wmean"]), len(bad["winner"])))
    assert not bad["wmean"], ("centroid bits differ (set)", bad["wmean"])
    assert not bad["mind"], ("min(dl, dr) bits differ (set, candidate)", mind_elems, bad["mind"][:8])
    assert not bad["counts"], ("(n_left, n_right) differ (set, candidate)", bad["counts"][:8])
    assert not bad["lists"], ("member lists differ (set, candidate)", bad["lists"][:8])
    assert not bad["score"], ("score bits differ (set, candidate)", bad["score"][:8])
    assert not bad["winner"], ("the acceptance rule picks another candidate (set)", bad["winner"])


@pytest.mark.parametrize("n", kc.SIZES)
@pytest.mark.parametrize("kind", kc.FAMILIES)
def test_candidates_device_equals_host(ctx, kind, n):
    """a single set at the shape the product takes for it: <128, 32> up to 1024 samples, <512, 512> above"""
    _compare_level(ctx, kind, (n,), False)


@pytest.mark.parametrize("n", [n for n in kc.SIZES if n <= 1024])
@pytest.mark.parametrize("kind", kc.FAMILIES)
def test_candidates_device_equals_host_at_the_forced_big_shape(ctx, kind, n):
    """what the product runs small sets with whenever their level also holds a set above 1024"""
    _compare_level(ctx, kind, (n,), True)


@pytest.mark.parametrize("sizes", kc.MIXED_LEVELS)
@pytest.mark.parametrize("kind", kc.FAMILIES)
def test_candidates_of_mixed_levels(ctx, kind, sizes):
    """several sets in one launch: cand0, list_off and the scratch offsets away from zero, both shapes"""
    _compare_level(ctx, kind, sizes, False)


# ---- whole trees on constructed matrices, through the public entry point ----

LEN = 625                                      # (625 + 625) / 2 / 10000 = 0.0625 exactly: d_estimation's length term


def _identical(n):
    return [(np.arange(LEN) * 7 % 13).astype(np.uint8)] * n


def _tree(ctx, monkeypatch, M, km):
    """the guide tree of the matrix M (N x 32); km: "0" host, "1" device, None: the product's own choice"""
    from kalign_amd import api
    if km is None:
        monkeypatch.delenv("KA_KMEANS", raising=False)
    else:
        monkeypatch.setenv("KA_KMEANS", km)
    M = np.ascontiguousarray(M, np.float32)
    scale = np.float32(16.0) * M
    assert np.isfinite(scale).all()
    tasks, sd = ctx.guide_tree(_identical(len(M)), n_threads=4, dm_scale=scale)
    on_device = bool(api.guide_last_bisect()[1])
    # the injection itself: seq_distances is the row mean of the matrix the bisection saw, over the length
    mean = np.cumsum(M, axis=1, dtype=np.float32)[:, -1] / np.float32(kc.PAD)
    assert np.array_equal(_bits(sd), _bits(mean / np.float32(LEN)))
    return tasks, on_device


@pytest.mark.parametrize("n", (600, 2047, 2048, 2500))
@pytest.mark.parametrize("kind", kc.FAMILIES + ("peel",))
def test_tree_device_equals_host(ctx, monkeypatch, kind, n):
    M = kc.matrix(kind, n, 4000 + n)
    t_host, dev0 = _tree(ctx, monkeypatch, M, "0")
    t_dev, dev1 = _tree(ctx, monkeypatch, M, "1")
    assert not dev0 and dev1
    assert np.array_equal(t_host, t_dev)
    if kind == "peel":
        # lopsided on purpose, so that the case is not vacuous: an evenly splitting tree of these sizes is 12 to 14 nodes
        # deep (the family_like trees), here every row whose square is still finite costs a level of its own
        depth = np.zeros(2 * n - 1, np.int64)
        for a, b, c in t_dev[::-1]:
            depth[a] = depth[b] = depth[c] + 1
        assert depth.max() >= 30


@pytest.mark.parametrize("n,on_device", [(2047, False), (2048, True)])
def test_tree_default_threshold(ctx, monkeypatch, n, on_device):
    """without KA_KMEANS in the environment 2047 sequences bisect on the host and 2048 on the device; same trees"""
    M = kc.matrix("family_like", n, 5000 + n)
    t_default, dev = _tree(ctx, monkeypatch, M, None)
    assert dev == on_device
    t_other, dev_other = _tree(ctx, monkeypatch, M, "0" if on_device else "1")
    assert dev_other != on_device
    assert np.array_equal(t_default, t_other)


@pytest.mark.parametrize("n,seed,sigma", [(600, 11, 0.3), (2048, 12, 0.3), (1100, 13, 0.8)])
def test_tree_noise_blob_equals_the_reference(ctx, monkeypatch, n, seed, sigma):
    """the one family the reference can be given through its own entry point: build_tree_kmeans_noisy on identical
    sequences -- device tree == host tree == the real reference's tree"""
    from oracle import refdrv
    if not refdrv.available():
        pytest.skip("oracle/_ref not built")
    letters = "".join("ACDEFGHIKLMNPQRSTVWY"[(7 * k) % 20] for k in range(LEN))
    job = refdrv.RefJob([letters] * n, tree_seed=seed, tree_noise=sigma, n_threads=4)
    scale = refdrv.noise_multipliers(seed, sigma, n * kc.PAD)
    for km in ("0", "1"):
        monkeypatch.setenv("KA_KMEANS", km)
        tasks, sd = ctx.guide_tree(job.tree_codes, n_threads=4, dm_scale=scale)
        assert np.array_equal(tasks, job.tasks), km
        assert np.array_equal(_bits(sd), _bits(job.seq_distances)), km
    job.close()


def test_tree_edge_shapes_on_the_device(ctx, monkeypatch):
    """the shapes tests/test_guide_tree.py::test_live_edge_shapes runs through the host bisection -- exactly 50 and 51
    sequences, 128, many identical sequences, few distinct ones, two tight clusters, one long outlier -- through the
    device one, against the real build_tree_kmeans"""
    from oracle import refdrv
    from kalign_amd import api, synth
    if not refdrv.available():
        pytest.skip("oracle/_ref not built")
    rng = np.random.RandomState(9)
    fam = synth.family(60, 80, seed=31)
    a, b = synth.family(45, 60, seed=32), synth.family(45, 140, seed=33)
    cases = {
        "n50": synth.family(50, 60, seed=34), "n51": synth.family(51, 60, seed=35), "n128": synth.family(128, 40, seed=36),
        "identical": [fam[0]] * 70 + fam[:10],
        "few_distinct": [fam[i % 3] for i in range(90)],
        "two_clusters": a + b,
        "outlier": synth.family(80, 50, seed=37) + ["".join("ACDEFGHIKLMNPQRSTVWY"[k] for k in rng.randint(0, 20, size=900))],
    }
    monkeypatch.setenv("KA_KMEANS", "1")
    for name, seqs in cases.items():
        job = refdrv.RefJob(seqs)
        tasks, sd = ctx.guide_tree(job.tree_codes, n_threads=2)
        assert api.guide_last_bisect()[1], name
        assert np.array_equal(tasks, job.tasks), name
        assert np.array_equal(_bits(sd), _bits(job.seq_distances)), name
        job.close()


def test_tree_pool_reuse_large_small_large(ctx, monkeypatch):
    """the per-device buffer pool is reused and never shrinks: a small tree after a large one runs in the large one's
    buffers, and the large one again afterwards is what it was"""
    big = kc.matrix("noise_blob", 2500, 61)
    small = kc.matrix("family_like", 600, 62)
    t_big, _ = _tree(ctx, monkeypatch, big, "1")
    t_small, _ = _tree(ctx, monkeypatch, small, "1")
    t_big2, _ = _tree(ctx, monkeypatch, big, "1")
    assert np.array_equal(t_big, t_big2)
    assert np.array_equal(t_small, _tree(ctx, monkeypatch, small, "0")[0])
    assert np.array_equal(t_big, _tree(ctx, monkeypatch, big, "0")[0])


def test_tree_two_contexts_two_threads(ctx, monkeypatch):
    """two contexts on one device building different trees at once share the device's pool under its lock: each tree
    equals its serial result"""
    import kalign_amd
    mats = [kc.matrix("noise_blob", 2100, 71), kc.matrix("near_plane", 1300, 72)]
    serial = [_tree(ctx, monkeypatch, M, "1")[0] for M in mats]
    monkeypatch.setenv("KA_KMEANS", "1")
    others = [kalign_amd.Context(0), kalign_amd.Context(0)]
    got = [[], []]
    errors = []

    def work(k):
        try:
            for _ in range(3):
                M = mats[k]
                got[k].append(others[k].guide_tree(_identical(len(M)), n_threads=2, dm_scale=np.float32(16.0) * M)[0])
        except Exception as e:                      # reported below, in the test's thread
            errors.append(e)
    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for c in others:
        c.close()
    assert not errors, errors
    for k in range(2):
        assert len(got[k]) == 3
        for t in got[k]:
            assert np.array_equal(t, serial[k]), k
