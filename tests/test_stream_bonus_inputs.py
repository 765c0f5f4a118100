"""Host-only: the seeded jobs of tests/test_gpu_stream_bonus.py reach the states the streamed-bonus kernels exist for.

Conditions on the INPUTS, from the oracle's position maps through tests/bonus_restate.py: a later change of seeds or of the
generator cannot quietly reduce that suite to what the K <= 5 kernels could have done.  The restatement itself is held to the
oracle: the dense matrix it implies hashes to the oracle's bonus hash of every seq-seq task."""
import functools

import numpy as np

import bonus_restate as br
import stream_jobs as sj


@functools.lru_cache(maxsize=None)
def _measured(k, kind, *args):
    from oracle import oracledrv
    codes, tasks, dist, dna = getattr(sj, kind + "_job")(*args)
    subm, scal = sj.scoring(dna)
    _, _, _, ids, maps, bh = oracledrv.msa_tree_cons(codes, tasks, subm, scal, dist, k, 2.0)
    lens = [len(c) for c in codes]
    return ids, maps, lens, tasks, bh, br.stats(maps, lens, tasks)


def _boundary():
    return [_measured(k, "boundary", k) for k in sj.BOUNDARY_K]


def _k128():
    return [_measured(128, "k128", dna) for dna in (True, False)]


def test_restatement_gives_the_oracles_bonus_matrices(oracle):
    L = oracle.lib()
    for ids, maps, lens, tasks, bh, _ in _boundary() + [_measured(8, "shape", 200, 7, True), _measured(8, "shape", 1, 3, False)]:
        for t in br.seq_seq_tasks(tasks, len(lens)):
            rows, cols, lists = br.entries(maps, lens, int(tasks[t][0]), int(tasks[t][1]))
            dense = np.zeros((rows, cols), np.float32)
            for i, row in enumerate(lists):
                for j, v, _ in row:
                    if j < cols:
                        dense[i, j] = v
                    else:                                        # the wrap-around entry is the next row's first cell
                        assert lists[i + 1][0][0] == 0 and lists[i + 1][0][1] == v
            assert L.ko_fnv1a(dense.ctypes.data, 4 * rows * cols) == int(bh[t]), t


def test_every_job_has_more_than_five_anchors():
    for k, (ids, *_) in zip(sj.BOUNDARY_K, _boundary()):
        assert len(ids) == k
    for ids, *_ in _k128():
        assert len(ids) == 128
    assert len(_measured(128, "shape", 64, 64, False)[0]) == 8     # the cap: K = N
    assert len(_measured(11, "refine")[0]) == 11


def test_every_boundary_job_has_rows_with_more_than_five_entries():
    for k, m in zip(sj.BOUNDARY_K, _boundary()):
        assert m[5]["over5"] >= 5, (k, m[5])
    assert _measured(11, "refine")[5]["over5"] > 0


def test_128_anchor_jobs_have_a_row_with_at_least_sixteen_entries():
    for m in _k128():
        assert m[5]["longest"] >= 16, m[5]
        assert m[5]["longest"] + 1 + 2 + 2 <= 136                  # (KA_NB_BIG: the entries, the wrap-around one, sentinels, pads)


def test_rows_without_entries_summed_cells_and_wrap_around_entries_occur():
    stats = [m[5] for m in _boundary() + _k128()]
    assert any(s["empty"] > 0 for s in stats), stats
    assert any(s["summed"] > 0 for s in stats), stats
    assert any(s["wrap"] > 0 for s in stats), stats
    # ... and in one job together: lists that end on the sentinel at once beside lists the pad slot's entry joined
    assert any(s["empty"] > 0 and s["wrap"] > 0 and s["over5"] > 0 for s in stats), stats


def test_ragged_golden_has_tasks_of_1_65_128_and_129_rows():
    """the strip edges of the streamed kernels: the stored file, not the recipe, is what the GPU tests run"""
    from util import Golden
    g = Golden("cons_stream_ragged_k6")
    assert len(g.anchor_ids) == 6
    rows = {int(lb if sw else la) for la, lb, sw in zip(g.rec("len_a"), g.rec("len_b"), g.rec("swapped"))}
    assert {1, 65, 128, 129} <= rows, sorted(rows)
    assert max(rows) > 256                                         # (and a task of three strips)


def test_shape_list_has_one_row_tasks():
    n = sum(_measured(8, "shape", la, lb, dna)[5]["one_row_tasks"] for la, lb in sj.SHAPES[:10] for dna in (False, True))
    assert n > 0

