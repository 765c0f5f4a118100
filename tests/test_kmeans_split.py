"""The host's split2 (ka_guide.cpp, through ka_debug_kmeans_host) against the REAL split2 of the reference
(bisectingKmeans.c:766-971, compiled with its own AVX2 edist_256 into oracle/_ref; oracle/ref_split_harness.c), candidate
by candidate: the score by its bits, counts and both lists exactly, for every seed bisecting_kmeans tries.  CPU only.
The device's candidates are compared with the host's in tests/test_gpu_kmeans.py; this file is what makes the host side
an oracle at the level of a rounding, where a finished tree is blind."""
import numpy as np
import pytest

import kmeans_cases as kc


def _ref_or_skip():
    from oracle import refdrv
    if not refdrv.has_split():
        pytest.skip("oracle/_ref not built (or built without ref_split_harness.c)")
    return refdrv


def _compare_with_reference(refdrv, dm, smp, cands, what):
    score, counts, lists = refdrv.split_all(dm, smp)
    assert len(cands) == len(score)
    for c, h in enumerate(cands):
        assert np.float32(h["score"]).view(np.uint32) == score[c].view(np.uint32), (what, c, h["score"], score[c])
        assert tuple(h["counts"]) == tuple(counts[c]), (what, c)
        assert np.array_equal(h["sl"], lists[c, 0, :counts[c, 0]]), (what, c)
        assert np.array_equal(h["sr"], lists[c, 1, :counts[c, 1]]), (what, c)


@pytest.mark.parametrize("n", kc.SIZES)
@pytest.mark.parametrize("kind", kc.FAMILIES)
def test_host_split_equals_the_reference_split(kind, n):
    refdrv = _ref_or_skip()
    dm, samples, sets, host = kc.host_level(kind, (n,))
    start = int(sets[0][0])
    _compare_with_reference(refdrv, dm, samples[start:start + n], host[0], (kind, n))


@pytest.mark.parametrize("sizes", kc.MIXED_LEVELS)
@pytest.mark.parametrize("kind", ("family_like", "near_plane", "noise_blob"))
def test_host_split_equals_the_reference_split_on_mixed_levels(kind, sizes):
    refdrv = _ref_or_skip()
    dm, samples, sets, host = kc.host_level(kind, sizes)
    for k, (start, n) in enumerate(sets):
        _compare_with_reference(refdrv, dm, samples[start:start + n], host[k], (kind, sizes, k))


@pytest.mark.parametrize("n", kc.SIZES)
@pytest.mark.parametrize("kind", kc.FAMILIES)
def test_every_family_reaches_its_branch(kind, n):
    """no GPU and no reference needed: the counters of the host seam show that near_plane mixes parity and distance
    decisions in one run, all_equal is the parity rule alone, swamped ends in the degenerate cut in every candidate and
    the noise blob runs long (20 iterations and more from 513 samples on)"""
    _, _, _, host = kc.host_level(kind, (n,))
    kc.check_conditions(kind, n, host[0])
    for h in host[0]:
        assert h["counts"].sum() == n and 1 <= h["iterations"] <= 500
        if h["degenerate"]:
            assert h["score"] == 0.0 and tuple(h["counts"]) == (n // 2, n - n // 2)


def test_the_iteration_cap_is_not_reached_by_these_families():
    """split2 stops after 500 iterations whatever the centroids do; no input of these families gets there (the longest run
    is reported), so the cap itself stays untested"""
    longest = 0
    for kind in kc.FAMILIES:
        for n in kc.SIZES:
            longest = max(longest, max(h["iterations"] for h in kc.host_level(kind, (n,))[3][0]))
    print("longest 2-means run: %d iterations" % longest)
    assert longest < 500
